"""CRF refinement of a prediction under the frame it was made from: windowed mean-field inference on the device.  An EXTENSION:
the reference has no counterpart.  The model is the fully connected CRF of Kraehenbuehl & Koltun 2011 with the message passing
restricted to a local window, ConvCRF (Teichmann & Cipolla 2018): an exact, deterministic, dense stencil.

Every other treatment of a teacher's prediction here reads labels or scores alone (``pseudo``, ``proto``, ``boundary.erode``,
``regions.sieve``, ``calibration``); the decoder up-samples by nearest x2, so a label boundary sits on a blurred staircase, not on
the edge the frame shows.  ``refine`` moves it there: a pixel's class distribution is pulled towards those of the pixels of its
window that look like it.

The rule (part of the public contract; ``include/udaseg.h`` states it in full, ``tests/_crf_ref.py`` is its numpy mirror)
    ``P0 = softmax(scores)`` (or the scores themselves, renormalised, with ``probs``).  Neighbours of pixel ``i``:
    ``j = i + dilation * (dy, dx)``, ``|dy|, |dx| <= radius``, not ``(0, 0)``, inside the same image and valid.
    ``k_ij = w_app * exp(-|p_i - p_j|^2 / (2 theta_alpha^2)) * exp(-|I_i - I_j|^2 / (2 theta_beta^2))
    + w_smooth * exp(-|p_i - p_j|^2 / (2 theta_gamma^2))``; ``Z_i`` is the same sum without the colour factor;
    ``m_i(c) = strength * sum_j k_ij Q_j(c) / Z_i``; ``Q <- softmax(log P0 + m)``, ``iterations`` Jacobi sweeps from ``Q = P0``.
    A pixel whose row is not finite (``probs``: not in ``[0, 1]``, or of sum 0) is void: a NaN row, no message sent, no mass.

Two kernels (csrc/crf.hip): ``udaseg_crf_prepare`` once, ``udaseg_crf_step`` once per sweep, ping-pong between two buffers.  No
sort, no atomics, no host read, no gradient: two calls give the same bits.  No CPU path.

Use::

    probs = crf.refine(model(images), frames_u8)                       # [N,C,H,W] probabilities; consumers take probs=True
    labels, conf = crf.refine_labels(model(images), frames_u8)
    labeler = crf.CrfLabeler(mean_teacher, num_classes=23, portion=0.2, cap=0.9)       # an OnlineLabeler; .loader() as usual
    labels = crf.refine_large(model, frame_u8_hwc, tile=512, tta="flips", iterations=5)
"""
import numpy as np
import torch

from . import _args as A
from . import kernels as K
from . import pseudo, teacher
from .engine import ceil4

MAX_RADIUS, MAX_DILATION, MAX_REACH, MAX_ITERATIONS = 5, 4, 10, 16
# ConvCRF's published settings: appearance weight 10 with position scale 80 and colour scale 13, smoothness weight 3 with position
# scale 3.  Nobody has tuned them on this data.
DEFAULTS = dict(radius=3, dilation=2, iterations=5, w_app=10.0, w_smooth=3.0, theta_alpha=80.0, theta_beta=13.0, theta_gamma=3.0,
                strength=1.0)


def check_params(radius=3, dilation=2, iterations=5, w_app=10.0, w_smooth=3.0, theta_alpha=80.0, theta_beta=13.0, theta_gamma=3.0,
                 strength=1.0):
    """The parameters as a dict of plain numbers; ``ValueError`` for one outside its range (module docstring, ``udaseg.h``)."""
    who = "crf"
    p = dict(radius=A.int_in(who, "radius", radius, 1, MAX_RADIUS), dilation=A.int_in(who, "dilation", dilation, 1, MAX_DILATION),
             iterations=A.int_in(who, "iterations", iterations, 0, MAX_ITERATIONS),
             w_app=A.number(who, "w_app", w_app, 0.0), w_smooth=A.number(who, "w_smooth", w_smooth, 0.0),
             theta_alpha=A.number(who, "theta_alpha", theta_alpha, 0.0, lo_open=True),
             theta_beta=A.number(who, "theta_beta", theta_beta, 0.0, lo_open=True),
             theta_gamma=A.number(who, "theta_gamma", theta_gamma, 0.0, lo_open=True),
             strength=A.number(who, "strength", strength, 0.0))
    if p["radius"] * p["dilation"] > MAX_REACH:
        raise ValueError(f"radius * dilation must not exceed {MAX_REACH}, got {p['radius']} * {p['dilation']}")
    if p["w_app"] == 0.0 and p["w_smooth"] == 0.0:
        raise ValueError("w_app and w_smooth must not both be 0")
    with np.errstate(over="ignore"):
        inv2b = inv2b_of(p["theta_beta"])
    if not (np.isfinite(inv2b) and inv2b > 0):
        raise ValueError(f"theta_beta = {theta_beta!r}: 1 / (2 theta_beta^2) is not a positive fp32 number")
    return p


def spatial_table(radius, dilation, theta):
    """fp32 ``[(2 radius + 1)^2]``: ``exp(-(dy^2 + dx^2) dilation^2 / (2 theta^2))`` in float64, rounded; row ``dy + radius``."""
    o = np.arange(-radius, radius + 1, dtype=np.float64)
    r2 = (o[:, None] ** 2 + o[None, :] ** 2) * float(dilation) ** 2
    return np.exp(-r2 / (2.0 * float(theta) ** 2)).astype(np.float32).reshape(-1)


def inv2b_of(theta_beta):
    """``fp32(1 / (2 theta_beta^2))``, the colour term's factor as the kernel receives it."""
    return np.float32(1.0 / (2.0 * float(theta_beta) ** 2))


@torch.no_grad()
def refine(outputs, frames_u8, radius=3, dilation=2, iterations=5, w_app=10.0, w_smooth=3.0, theta_alpha=80.0, theta_beta=13.0,
           theta_gamma=3.0, strength=1.0, probs=False, out=None):
    """``[N,C,H,W]`` fp32 probabilities of ``[N,C,H,W]`` logits (or probabilities with ``probs``) refined under the uint8
    ``[N,H,W,3]`` frames by ``iterations`` mean-field sweeps (module docstring).  The result is a strided view of a padded NHWC
    buffer, the form ``proto.rectify`` returns: ``ConfidenceHistogram.update``, ``pseudo_labels``, ``confidence_share``,
    ``SoftCrossEntropyLoss``, ``calibration`` and the ``boundary`` / ``regions`` statistics read it in place with ``probs=True``.
    Void pixels are NaN rows.  ``out``: an fp32 ``[N,H,W,ceil4(C)]`` contiguous device tensor to hold the result, or None.

    The defaults follow ConvCRF's published ratio of appearance to smoothness weight and its colour scale; NOBODY HAS TUNED THEM ON
    THIS DATA.  ``iterations = 0`` returns ``P0``.  ``1 + iterations`` launches, no gradient, no host read; bad parameters raise
    ``ValueError`` before any launch, CPU tensors raise ``RuntimeError``."""
    p = check_params(radius, dilation, iterations, w_app, w_smooth, theta_alpha, theta_beta, theta_gamma, strength)
    n, c, h, w = A.scores_shape("refine", outputs)
    A.frames_u8("refine", frames_u8, (n, h, w))
    ldq = ceil4(c)
    dev = A.same_gpu("refine", scores=outputs, frames=frames_u8)
    out = A.out_tensor("refine", "out", out, (n, h, w, ldq), torch.float32, dev, contiguous=True)
    return A.on_device(dev, _refine, p, outputs, frames_u8.contiguous(), probs, out, n, c, h, w, ldq)


def _refine(p, outputs, frames, probs, out, n, c, h, w, ldq):
    """``refine``'s launches on checked operands, the scores' device current."""
    dev = outputs.device
    sbuf, ldc = A.padded_nhwc(outputs.detach())
    T = p["iterations"]
    logp = torch.empty((n, h, w, ldq), dtype=torch.float32, device=dev)
    valid = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    other = torch.empty_like(out) if T > 0 else None
    cur, nxt = (out, other) if T % 2 == 0 else (other, out)        # the last sweep lands in out
    K.crf_prepare(sbuf, ldc, c, probs, n * h * w, logp, cur, ldq, valid)
    if T > 0:
        sa = torch.from_numpy(spatial_table(p["radius"], p["dilation"], p["theta_alpha"])).to(dev)
        sg = torch.from_numpy(spatial_table(p["radius"], p["dilation"], p["theta_gamma"])).to(dev)
        inv2b = float(inv2b_of(p["theta_beta"]))
        for _ in range(T):
            K.crf_step(logp, cur, valid, frames, c, ldq, p["radius"], p["dilation"], sa, sg, p["w_app"], p["w_smooth"], inv2b,
                       p["strength"], nxt)
            cur, nxt = nxt, cur
    return out.permute(0, 3, 1, 2)[:, :c]


def _zero_thresholds(classes, device):
    return torch.zeros(classes, dtype=torch.int32, device=device)


def refine_labels(outputs, frames_u8, void=255, probs=False, **crf_kwargs):
    """``(labels uint8 [N,H,W], confidence fp32 [N,H,W])`` of ``refine``'s probabilities: the first maximal class (THE tie rule of
    ``pseudo_labels`` and ``predict_large``) and its probability; ``void`` and 0 at a void pixel."""
    q = refine(outputs, frames_u8, probs=probs, **crf_kwargs)
    return pseudo.pseudo_labels(q, _zero_thresholds(q.shape[1], q.device), void, probs=True, return_confidence=True)


class CrfLabeler(teacher.OnlineLabeler):
    """``OnlineLabeler`` whose probabilities are refined under the frames: every ``label`` call makes ONE eval-mode, no-grad forward
    of the teacher, ``refine``s it with the frames it was made from, adds the refined probabilities to the confidence table, takes
    the thresholds from the table as it then stands and labels under them, all with ``probs=True``.  ``loader()`` is
    ``OnlineLabeler``'s: the ``SievedLoader`` / ``ErodedLoader`` / ``MixedLoader`` chains take it unchanged.  ``crf_kwargs``:
    ``refine``'s parameters (checked here)."""

    def __init__(self, teacher, num_classes, portion=0.2, floor=0.0, cap=0.9, bins=pseudo.BINS, void=255, halve_every=None,
                 dtype=None, **crf_kwargs):
        super().__init__(teacher, num_classes, portion, floor, cap, bins, void, halve_every, dtype)
        self.crf = check_params(**crf_kwargs)

    def label(self, frames_u8):
        """uint8 ``[N,H,W]`` masks (device) of uint8 ``[N,H,W,3]`` frames; updates the table and ``self.thr_bins``.  No host read."""
        q = refine(self._eval_forward(frames_u8), frames_u8, **self.crf)
        if self.halve_every and self.calls and self.calls % self.halve_every == 0:
            self.halve_(self.hist.table)
        self.calls += 1
        self.hist.update(q, probs=True)
        self.thr_bins = self.hist.thresholds(self.portion, self.floor, self.cap)
        return pseudo.pseudo_labels(q, self.thr_bins, self.void, probs=True, bins=self.bins)


def refine_large(model, frame_u8_hwc, return_probs=False, **kwargs):
    """Label map int64 ``[H,W]`` (and, with ``return_probs``, the refined ``[1,C,H,W]`` probabilities) of one frame of any size
    with ``H * W < 2^31``: ``predict_large(..., return_probs=True)``, then ONE ``refine`` of the whole blended frame, so no tile
    seam is visible in the refinement.  ``kwargs``: ``refine``'s parameters and ``predict_large``'s, told apart by name."""
    from .predict import predict_large
    crf_kwargs = check_params(**{k: kwargs.pop(k) for k in list(kwargs) if k in DEFAULTS})
    _, probs = predict_large(model, frame_u8_hwc, return_probs=True, **kwargs)
    frame = frame_u8_hwc
    if isinstance(frame, np.ndarray):
        frame = torch.from_numpy(np.ascontiguousarray(frame))
    frame = frame.to(probs.device, non_blocking=True)[None]
    q = refine(probs, frame, probs=True, **crf_kwargs)
    _, c, h, w = q.shape
    labels = torch.empty((h, w), dtype=torch.int64, device=q.device)
    qbuf, ldq = A.padded_nhwc(q)                                   # the buffer q is a view of (no launch)
    A.on_device(q.device, K.predict_finish, qbuf, None, h * w, c, ldq, labels)
    return (labels, q) if return_probs else labels


__all__ = ["refine", "refine_labels", "refine_large", "CrfLabeler", "check_params", "spatial_table", "inv2b_of", "DEFAULTS"]
