"""Loss modules of the hot path, backed by the wavefront-reduced HIP kernels in csrc/losses.hip.

* ``CrossEntropyLoss``  -- ``nn.CrossEntropyLoss()`` exactly as the reference constructs it (no arguments: mean
  reduction, no class weights, no ignore_index, no label smoothing; reference ``src/models/train.py:208``); with
  ``weight`` / ``ignore_index`` / ``reduction`` / ``label_smoothing`` the optioned kernels (void labels).
* ``OhemCrossEntropyLoss``, ``TopKCrossEntropyLoss`` -- the cross entropy over the hard pixels only (online hard example mining /
  bootstrapped top-k; an extension), selected exactly on the device by a radix select (csrc/ohem.hip; INTEGRATION.md
  "Hard-pixel mining").
* ``LovaszSoftmaxLoss`` -- the Lovasz-softmax Jaccard surrogate (Berman et al. 2018; an extension), on integer error histograms
  instead of a sort, with a reported bound on what the grid costs (csrc/lovasz.hip; INTEGRATION.md "Lovasz-softmax").
* ``AdversarialLoss``   -- mirror of reference ``src/models/losses.py:7-51`` (same constructor, same two methods).
  As upstream, BCE-*with-logits* is applied to whatever the discriminator returns (its sigmoid output).
* ``DiceLoss``, ``WeightedSegmentationLoss``, ``ConsistencyLoss``, ``FineTuningLoss``, ``calculate_class_weights`` --
  the rest of the reference's loss family (``src/models/losses.py:53-342``), kernels in
  csrc/losses_seg.hip: one pass over the logits per direction, softmax rows in registers.
"""
from typing import Dict, Optional
import os

import torch
import torch.nn as nn

from . import kernels as K
from ._args import padded_nhwc
from ._lib import load as _load


# the training step's loss makes its gradient in the forward pass (one read of the logits instead of two); UDASEG_FUSE_CE=0: two passes
FUSE_CE_BACKWARD = os.environ.get("UDASEG_FUSE_CE", "1") != "0"
# data_ptr of the last dlogits buffer -> its per-class column sums (consumed once by Unet._backward_plan)
COLSUM_SIDE_TABLE = {}


class _CrossEntropyFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        n, c, h, w = logits.shape
        buf, ldc = padded_nhwc(logits.detach())
        tgt = target.contiguous()
        pixels = n * h * w
        dev = logits.device
        partials = torch.empty(_load().udaseg_ce_partials(), device=dev, dtype=torch.float64)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        ctx.meta = (n, c, h, w, ldc)
        ctx.fused = None
        if FUSE_CE_BACKWARD and ldc <= 32 and ctx.needs_input_grad[0]:
            # a training step: the gradient for an upstream gradient of 1 (what loss.backward() passes) is made in the SAME pass over
            # the logits as the loss, with the head's bias gradient (column sums); backward() only scales it if it has to
            dl = torch.empty((n, h, w, ldc), device=dev, dtype=torch.float32)
            parts = torch.empty(_load().udaseg_ce_partials() * ldc, device=dev, dtype=torch.float32)
            colsum = torch.empty(ldc, device=dev, dtype=torch.float32)
            K.ce_fwd_bwd(buf, tgt, pixels, c, ldc, partials, loss, dl, parts, colsum)
            ctx.fused = [dl, colsum]
            ctx.save_for_backward(buf, tgt)
            return loss
        lse = torch.empty(pixels, device=dev, dtype=torch.float32)
        K.ce_fwd(buf, tgt, pixels, c, ldc, lse, partials, loss)
        ctx.save_for_backward(buf, tgt, lse)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        n, c, h, w, ldc = ctx.meta
        g = grad_out.detach().to(torch.float32).contiguous()
        if ctx.fused is not None:
            dl, colsum = ctx.fused
            ctx.fused = None                           # consumed (a second backward through a retained graph takes the two-pass route)
            K.scale_unless_one(dl, g, colsum)
            COLSUM_SIDE_TABLE.clear()
            COLSUM_SIDE_TABLE[dl.data_ptr()] = colsum
            return dl.permute(0, 3, 1, 2)[:, :c], None
        if len(ctx.saved_tensors) == 2:                # fused forward, second backward: recompute the log-sum-exp
            buf, tgt = ctx.saved_tensors
            lse = torch.empty(n * h * w, device=buf.device, dtype=torch.float32)
            K.ce_fwd(buf, tgt, n * h * w, c, ldc, lse, torch.empty(_load().udaseg_ce_partials(), device=buf.device, dtype=torch.float64),
                     torch.empty((), device=buf.device, dtype=torch.float32))
        else:
            buf, tgt, lse = ctx.saved_tensors
        dl = torch.empty((n, h, w, ldc), device=buf.device, dtype=torch.float32)
        out = dl.permute(0, 3, 1, 2)[:, :c]
        if ldc <= 32:
            # per-class sums of the gradient come out of the same pass: the head conv's bias gradient (Unet's backward
            # plan picks it up from the side table instead of re-reading the 200 MB gradient)
            parts = torch.empty(_load().udaseg_ce_partials() * ldc, device=buf.device, dtype=torch.float32)
            colsum = torch.empty(ldc, device=buf.device, dtype=torch.float32)
            K.ce_bwd(buf, tgt, lse, g, n * h * w, c, ldc, dl, parts, colsum)
            COLSUM_SIDE_TABLE.clear()
            COLSUM_SIDE_TABLE[dl.data_ptr()] = colsum
        else:
            K.ce_bwd(buf, tgt, lse, g, n * h * w, c, ldc, dl)
        return out, None


class _CrossEntropyOptFunction(torch.autograd.Function):
    """Cross entropy with class weights / ignore_index / label smoothing / a reduction (csrc/losses.hip, ce_opt_* kernels).

    One launch over the targets alone makes D (the 'mean' denominator, f64) and the target counters; then a training step reads
    the logits once and writes the gradient once, already scaled (``ce_opt_fwd_bwd``), with the head's bias gradient (column
    sums).  The two-pass route (forward keeping the log-sum-exp, then backward) serves no_grad forwards, ldc > 32, reduction
    'none' (its upstream gradient is a per-pixel map) and a second backward through a retained graph."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, reduction, eps, stats):
        n, c, h, w = logits.shape
        buf, ldc = padded_nhwc(logits.detach())
        tgt = target.contiguous()
        pixels = n * h * w
        dev = logits.device
        np_ = _load().udaseg_ce_partials()
        denom = torch.empty(1, device=dev, dtype=torch.float64)
        K.ce_target_stats(tgt, weight, pixels, c, ignore_index, torch.empty(4 * np_, device=dev, dtype=torch.float64), denom, stats)
        mean = reduction == 'mean'
        partials = torch.empty(np_, device=dev, dtype=torch.float64)
        ctx.meta = (n, c, h, w, ldc, ignore_index, reduction, eps)
        ctx.fused = None
        if reduction == 'none':
            lse = torch.empty(pixels, device=dev, dtype=torch.float32)
            loss_px = torch.empty((n, h, w), device=dev, dtype=torch.float32)
            K.ce_opt_fwd(buf, tgt, weight, pixels, c, ldc, ignore_index, eps, False, None, lse, partials, None, loss_px)
            ctx.save_for_backward(buf, tgt, weight, denom, lse)
            return loss_px
        loss = torch.empty((), device=dev, dtype=torch.float32)
        if FUSE_CE_BACKWARD and ldc <= 32 and ctx.needs_input_grad[0]:
            dl = torch.empty((n, h, w, ldc), device=dev, dtype=torch.float32)
            parts = torch.empty(np_ * ldc, device=dev, dtype=torch.float32)
            colsum = torch.empty(ldc, device=dev, dtype=torch.float32)
            K.ce_opt_fwd_bwd(buf, tgt, weight, pixels, c, ldc, ignore_index, eps, mean, denom, partials, loss, dl, parts, colsum)
            ctx.fused = [dl, colsum]
            ctx.save_for_backward(buf, tgt, weight, denom)
            return loss
        lse = torch.empty(pixels, device=dev, dtype=torch.float32)
        K.ce_opt_fwd(buf, tgt, weight, pixels, c, ldc, ignore_index, eps, mean, denom, lse, partials, loss, None)
        ctx.save_for_backward(buf, tgt, weight, denom, lse)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        n, c, h, w, ldc, ignore_index, reduction, eps = ctx.meta
        pixels = n * h * w
        g = grad_out.detach().to(torch.float32).contiguous()
        if ctx.fused is not None:
            dl, colsum = ctx.fused
            ctx.fused = None                           # consumed (a second backward takes the two-pass route)
            K.scale_unless_one(dl, g, colsum)
            COLSUM_SIDE_TABLE.clear()
            COLSUM_SIDE_TABLE[dl.data_ptr()] = colsum
            return (dl.permute(0, 3, 1, 2)[:, :c],) + (None,) * 6
        mean = reduction == 'mean'
        if len(ctx.saved_tensors) == 4:                # fused forward, second backward: recompute the log-sum-exp
            buf, tgt, weight, denom = ctx.saved_tensors
            lse = torch.empty(pixels, device=buf.device, dtype=torch.float32)
            K.ce_opt_fwd(buf, tgt, weight, pixels, c, ldc, ignore_index, eps, mean, denom, lse,
                         torch.empty(_load().udaseg_ce_partials(), device=buf.device, dtype=torch.float64),
                         torch.empty((), device=buf.device, dtype=torch.float32), None)
        else:
            buf, tgt, weight, denom, lse = ctx.saved_tensors
        g_scalar, g_px = (None, g.reshape(-1)) if reduction == 'none' else (g, None)
        dl = torch.empty((n, h, w, ldc), device=buf.device, dtype=torch.float32)
        if ldc <= 32:
            parts = torch.empty(_load().udaseg_ce_partials() * ldc, device=buf.device, dtype=torch.float32)
            colsum = torch.empty(ldc, device=buf.device, dtype=torch.float32)
            K.ce_opt_bwd(buf, tgt, weight, lse, g_scalar, g_px, pixels, c, ldc, ignore_index, eps, mean, denom, dl, parts, colsum)
            COLSUM_SIDE_TABLE.clear()
            COLSUM_SIDE_TABLE[dl.data_ptr()] = colsum
        else:
            K.ce_opt_bwd(buf, tgt, weight, lse, g_scalar, g_px, pixels, c, ldc, ignore_index, eps, mean, denom, dl)
        return (dl.permute(0, 3, 1, 2)[:, :c],) + (None,) * 6


class CrossEntropyLoss(nn.Module):
    """Per-pixel cross entropy over ``[N,C,H,W]`` logits and ``[N,H,W]`` integer targets, ``nn.CrossEntropyLoss``'s arguments.

    ``CrossEntropyLoss()`` is the plain loss the reference constructs (mean, no weights, no void handling): the plain kernels,
    one fused pass in a training step.  Any argument selects the optioned kernels, whose definition is
    ``torch.nn.functional.cross_entropy(input, target, weight, ignore_index=..., reduction=..., label_smoothing=...)``:
    a pixel is *valid* when ``target != ignore_index`` and ``0 <= target < C``; every other pixel is void: loss and gradient
    exactly 0 there, and 'mean' divides by the sum of ``weight[target]`` over the valid pixels only (all void: NaN loss, zero
    gradient, as torch; 'sum': 0).  ``reduction='none'`` returns fp32 ``[N,H,W]``.

    Two departures from torch:

    * ``ignore_index`` defaults to ``None`` ("no void handling", the plain route), not to ``-100``.  Any explicit value, ``-100``
      included, selects the optioned route.
    * An out-of-range target that is not ``ignore_index`` raises no ``IndexError`` (that needs a host read of every mask); it is
      treated as void and counted.  ``last_target_stats`` is a device int64 tensor ``[n_valid, n_void, n_invalid]`` of the last
      optioned call (``None`` on the plain route), written by the loss's own launches: read it when convenient.

    Under data parallelism each rank divides by its own D, as torch's DistributedDataParallel does.
    """

    def __init__(self, weight=None, ignore_index=None, reduction='mean', label_smoothing=0.0):
        super().__init__()
        if reduction not in ('none', 'sum', 'mean'):
            raise ValueError(f"CrossEntropyLoss: reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"CrossEntropyLoss: label_smoothing must lie in [0, 1], got {label_smoothing}")
        if weight is not None:
            weight = torch.as_tensor(weight)
            if weight.dim() != 1 or weight.numel() == 0:
                raise ValueError(f"CrossEntropyLoss: weight must be a 1-D tensor of C class weights, got shape {tuple(weight.shape)}")
            if weight.numel() > 64:
                raise ValueError(f"CrossEntropyLoss: at most 64 classes are supported by the HIP kernels, got {weight.numel()} weights")
            weight = weight.detach().to(torch.float32).clone()
        ignore_index = _check_ignore_index("CrossEntropyLoss", ignore_index)
        self.register_buffer('weight', weight)
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = float(label_smoothing)
        self.last_target_stats = None

    @property
    def route(self):
        """'plain': the kernels of ``CrossEntropyLoss()`` exactly as before; 'options': the ce_opt_* kernels."""
        plain = self.weight is None and self.ignore_index is None and self.reduction == 'mean' and self.label_smoothing == 0.0
        return 'plain' if plain else 'options'

    def extra_repr(self):
        return f"ignore_index={self.ignore_index}, reduction={self.reduction!r}, label_smoothing={self.label_smoothing}, route={self.route}"

    def forward(self, input, target):
        if input.device.type != "cuda":
            raise RuntimeError("CrossEntropyLoss: logits must live on the GPU (no CPU path in this build)")
        if input.dim() != 4 or target.dim() != 3 or input.shape[0] != target.shape[0] or input.shape[2:] != target.shape[1:]:
            raise ValueError(f"expected logits [N,C,H,W] and target [N,H,W]; got {tuple(input.shape)} and {tuple(target.shape)}")
        if target.dtype != torch.int64:
            target = target.long()
        if self.route == 'plain':
            return _CrossEntropyFunction.apply(input, target)
        c = input.shape[1]
        if c > 64:
            raise ValueError(f"CrossEntropyLoss: at most 64 classes are supported by the HIP kernels, got {c}")
        weight = self.weight
        if weight is not None:
            if weight.numel() != c:
                raise ValueError(f"CrossEntropyLoss: weight has {weight.numel()} entries for {c} classes")
            weight = weight.to(device=input.device, dtype=torch.float32).contiguous()
        stats = torch.empty(3, device=input.device, dtype=torch.int64)
        out = _CrossEntropyOptFunction.apply(input, target.to(input.device), weight, self.ignore_index, self.reduction,
                                             self.label_smoothing, stats)
        self.last_target_stats = stats
        return out


class _OhemCrossEntropyFunction(torch.autograd.Function):
    """Cross entropy over the hard pixels (csrc/ohem.hip).  One pass over the logits makes the target class's confidence per pixel
    and its level-0 histogram; a three-level radix select finds the exact k-th smallest confidence on the device; one pass over the
    confidences makes the 'mean' denominator and the counters; then ``ce_ohem_fwd_bwd`` reads the logits once more and writes the
    loss and the gradient, already scaled, with the head's bias gradient (column sums).  ``ws``: the zeroed int64 workspace
    [3 * 1024 histogram bins | 8 words of select state | 5 statistics]."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, mean, thresh, min_kept, fraction, ws, thr, keep):
        n, c, h, w = logits.shape
        buf, ldc = padded_nhwc(logits.detach())
        tgt = target.contiguous()
        pixels = n * h * w
        dev = logits.device
        np_ = _load().udaseg_ce_partials()
        nb = 3 * K.KTH_BINS
        hist, state, stats = ws[:nb].view(3, K.KTH_BINS), ws[nb:nb + K.KTH_STATE], ws[nb + K.KTH_STATE:]
        conf = torch.empty(pixels, device=dev, dtype=torch.float32)
        K.ohem_conf(buf, tgt, pixels, c, ldc, ignore_index, conf, hist[0], stats[2:5])
        K.kth_select(hist[0], 0, state, min_kept=min_kept, fraction=fraction)
        K.kth_refine(conf, hist, state)
        denom = torch.empty(1, device=dev, dtype=torch.float64)
        K.ohem_denom(conf, tgt, weight, pixels, c, thresh, state, torch.empty(3 * np_, device=dev, dtype=torch.float64), denom,
                     stats[0:2], keep)
        K.kth_value(state, thresh, thr)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        partials = torch.empty(np_, device=dev, dtype=torch.float64)
        ctx.meta = (n, c, h, w, ldc, mean, thresh)
        ctx.fused = None
        ctx.save_for_backward(buf, tgt, weight, conf, state, denom)
        if ctx.needs_input_grad[0]:
            dl, parts, colsum = _OhemCrossEntropyFunction._grad_buffers(n, h, w, ldc, np_, dev)
            K.ce_ohem_fwd_bwd(buf, tgt, weight, conf, state, thresh, pixels, c, ldc, mean, denom, partials, loss, dl, parts, colsum)
            ctx.fused = [dl, colsum]
        else:
            K.ce_ohem_fwd_bwd(buf, tgt, weight, conf, state, thresh, pixels, c, ldc, mean, denom, partials, loss)
        return loss

    @staticmethod
    def _grad_buffers(n, h, w, ldc, np_, dev):
        return (torch.empty((n, h, w, ldc), device=dev, dtype=torch.float32), torch.empty(np_ * ldc, device=dev, dtype=torch.float32),
                torch.empty(ldc, device=dev, dtype=torch.float32))

    @staticmethod
    def backward(ctx, grad_out):
        n, c, h, w, ldc, mean, thresh = ctx.meta
        g = grad_out.detach().to(torch.float32).contiguous()
        if ctx.fused is not None:
            dl, colsum = ctx.fused
            ctx.fused = None                           # consumed
        else:                                          # a second backward through a retained graph: the same launch on the saved
            buf, tgt, weight, conf, state, denom = ctx.saved_tensors      # conf and state, so the same kept set and the same bits
            np_ = _load().udaseg_ce_partials()
            dl, parts, colsum = _OhemCrossEntropyFunction._grad_buffers(n, h, w, ldc, np_, buf.device)
            K.ce_ohem_fwd_bwd(buf, tgt, weight, conf, state, thresh, n * h * w, c, ldc, mean, denom,
                              torch.empty(np_, device=buf.device, dtype=torch.float64),
                              torch.empty((), device=buf.device, dtype=torch.float32), dl, parts, colsum)
        K.scale_unless_one(dl, g, colsum)
        COLSUM_SIDE_TABLE.clear()
        COLSUM_SIDE_TABLE[dl.data_ptr()] = colsum
        return (dl.permute(0, 3, 1, 2)[:, :c],) + (None,) * 10


class OhemCrossEntropyLoss(nn.Module):
    """Per-pixel cross entropy over the HARD pixels only: online hard example mining (Shrivastava et al. 2016) in its per-pixel
    form, and with ``keep_fraction`` the bootstrapped / top-k cross entropy (Wu et al. 2016).  ``[N,C,H,W]`` logits (C <= 32) and
    ``[N,H,W]`` integer targets, as ``CrossEntropyLoss``.

    A pixel is *valid* as for ``CrossEntropyLoss`` (``target != ignore_index`` and ``0 <= target < C``); a valid pixel whose logits
    are not all finite is void as well (loss and gradient exactly 0) and counted on its own.  With ``p`` the softmax probability
    of the target class at a valid finite pixel and ``n`` the number of such pixels:

    * OHEM: a pixel is kept iff ``p < thresh`` or ``p <= q``, ``q`` the ``min_kept``-th smallest ``p`` -- the pixels below the
      threshold, but at least ``min(min_kept, n)`` of them.
    * top-k (``keep_fraction=f`` in (0, 1]): kept iff ``p <= q``, ``q`` the ``ceil(f * n)``-th smallest ``p``.

    ``q`` is exact (a radix select on the device: no sort, no bins, nothing read back, the same bits on every run) and pixels that
    tie with ``q`` are all kept, so the kept set depends on the values alone.  The loss is ``-weight[t] * log_softmax(z)[t]`` over
    the kept pixels; 'mean' divides by the sum of ``weight[t]`` over them (no kept pixel: NaN loss and an all-zero gradient, the
    convention of ``CrossEntropyLoss`` for an all-void batch; 'sum': 0).  The gradient is exactly 0 at every pixel not kept.
    Label smoothing is not supported: selection statistic and loss would no longer be monotone in each other.

    After a call, all on the device and written by the loss's own launches (read them when convenient):

    * ``last_ohem_stats``: int64 ``[n_valid_finite, n_kept, n_void, n_invalid, n_nonfinite]``;
    * ``last_threshold``: fp32 ``[q, max(q, thresh)]`` (``q`` is -inf when k == 0 and +inf when k > n);
    * ``last_keep_mask``: uint8 ``[N,H,W]``, made only with ``keep_mask=True``.

    Under data parallelism each rank selects on its own batch (its own ``n``, ``q`` and denominator), as each rank of torch's
    DistributedDataParallel divides by its own count.
    """

    def __init__(self, thresh=0.7, min_kept=100_000, keep_fraction=None, weight=None, ignore_index=None, reduction='mean',
                 keep_mask=False, label_smoothing=0.0):
        super().__init__()
        who = type(self).__name__
        if float(label_smoothing) != 0.0:
            raise ValueError(f"{who}: label smoothing is not supported (the selection statistic and the loss would no longer be "
                             f"monotone in each other), got {label_smoothing}")
        if reduction not in ('sum', 'mean'):
            raise ValueError(f"{who}: reduction must be 'sum' or 'mean', got {reduction!r}")
        if keep_fraction is not None:
            if thresh != 0.7 or min_kept != 100_000:
                raise ValueError(f"{who}: keep_fraction (top-k mode) excludes thresh and min_kept")
            if not 0.0 < float(keep_fraction) <= 1.0:
                raise ValueError(f"{who}: keep_fraction must lie in (0, 1], got {keep_fraction}")
            thresh, min_kept, keep_fraction = 0.0, 0, float(keep_fraction)
        else:
            if not 0.0 <= float(thresh) <= 1.0:
                raise ValueError(f"{who}: thresh must lie in [0, 1], got {thresh}")
            if isinstance(min_kept, bool) or int(min_kept) != min_kept or not 0 <= int(min_kept) < 2 ** 63:
                raise ValueError(f"{who}: min_kept must be a non-negative integer, got {min_kept!r}")
        if weight is not None:
            weight = torch.as_tensor(weight)
            if weight.dim() != 1 or weight.numel() == 0:
                raise ValueError(f"{who}: weight must be a 1-D tensor of C class weights, got shape {tuple(weight.shape)}")
            if weight.numel() > 32:
                raise ValueError(f"{who}: at most 32 classes are supported by the HIP kernels, got {weight.numel()} weights")
            weight = weight.detach().to(torch.float32).clone()
        self.register_buffer('weight', weight)
        self.thresh, self.min_kept, self.keep_fraction = float(thresh), int(min_kept), keep_fraction
        self.ignore_index = _check_ignore_index(who, ignore_index)
        self.reduction = reduction
        self.keep_mask = bool(keep_mask)
        self.last_ohem_stats = self.last_threshold = self.last_keep_mask = None

    def extra_repr(self):
        mode = f"keep_fraction={self.keep_fraction}" if self.keep_fraction is not None else f"thresh={self.thresh}, min_kept={self.min_kept}"
        return f"{mode}, ignore_index={self.ignore_index}, reduction={self.reduction!r}"

    def forward(self, input, target):
        who = type(self).__name__
        if input.device.type != "cuda":
            raise RuntimeError(f"{who}: logits must live on the GPU (no CPU path in this build)")
        if input.dim() != 4 or target.dim() != 3 or input.shape[0] != target.shape[0] or input.shape[2:] != target.shape[1:]:
            raise ValueError(f"expected logits [N,C,H,W] and target [N,H,W]; got {tuple(input.shape)} and {tuple(target.shape)}")
        n, c, h, w = input.shape
        if c > 32:
            raise ValueError(f"{who}: at most 32 classes are supported by the HIP kernels, got {c}")
        if n * h * w >= 2 ** 31:
            raise ValueError(f"{who}: at most 2^31 - 1 pixels per call, got {n * h * w}")
        if target.dtype != torch.int64:
            target = target.long()
        weight = self.weight
        if weight is not None:
            if weight.numel() != c:
                raise ValueError(f"{who}: weight has {weight.numel()} entries for {c} classes")
            weight = weight.to(device=input.device, dtype=torch.float32).contiguous()
        dev = input.device
        ws = torch.zeros(3 * K.KTH_BINS + K.KTH_STATE + 5, device=dev, dtype=torch.int64)
        thr = torch.empty(2, device=dev, dtype=torch.float32)
        keep = torch.empty((n, h, w), device=dev, dtype=torch.uint8) if self.keep_mask else None
        fraction = -1.0 if self.keep_fraction is None else self.keep_fraction
        out = _OhemCrossEntropyFunction.apply(input, target.to(dev), weight, self.ignore_index, self.reduction == 'mean', self.thresh,
                                              self.min_kept, fraction, ws, thr, keep)
        self.last_ohem_stats = ws[3 * K.KTH_BINS + K.KTH_STATE:]
        self.last_threshold = thr
        self.last_keep_mask = keep
        return out


class TopKCrossEntropyLoss(OhemCrossEntropyLoss):
    """The bootstrapped / top-k cross entropy: ``OhemCrossEntropyLoss(keep_fraction=...)``, the hardest ``ceil(keep_fraction * n)``
    of the ``n`` valid finite pixels (and every pixel that ties with the last of them)."""

    def __init__(self, keep_fraction, weight=None, ignore_index=None, reduction='mean', keep_mask=False):
        super().__init__(keep_fraction=keep_fraction, weight=weight, ignore_index=ignore_index, reduction=reduction,
                         keep_mask=keep_mask)


class _LovaszSoftmaxFunction(torch.autograd.Function):
    """Lovasz-softmax on a grid of error bins (csrc/lovasz.hip).  One pass over the logits makes the per-class fg / bg error
    histograms of every group; a tiny launch turns them into the Jaccard-gradient coefficient tables (reduction factor folded
    in), the present-class map and the grid bound; then ``lovasz_fwd_bwd`` reads the logits once more and writes the loss and
    the gradient with the head's bias gradient (column sums).  ``tables`` / ``counters`` come zeroed."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, images, bins, all_classes, ce_weight, tables, counters, present, slack):
        n, c, h, w = logits.shape
        buf, ldc = padded_nhwc(logits.detach())
        tgt = target.contiguous()
        pixels = n * h * w
        dev = logits.device
        np_ = _load().udaseg_ce_partials()
        K.lovasz_hist(buf, tgt, pixels, c, ldc, ignore_index, images, bins, tables, counters)
        coef = torch.empty(tables.shape, device=dev, dtype=torch.float32)
        K.lovasz_table(tables, images, c, bins, all_classes, coef, present, torch.empty(images * c, device=dev, dtype=torch.float64),
                       slack)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        partials = torch.empty(np_, device=dev, dtype=torch.float64)
        ctx.meta = (n, c, h, w, ldc, ignore_index, images, bins, ce_weight)
        ctx.fused = None
        ctx.save_for_backward(buf, tgt, coef, counters)
        if ctx.needs_input_grad[0]:
            dl, parts, colsum = _OhemCrossEntropyFunction._grad_buffers(n, h, w, ldc, np_, dev)
            K.lovasz_fwd_bwd(buf, tgt, coef, counters, pixels, c, ldc, ignore_index, images, bins, ce_weight, partials, loss, dl, parts,
                             colsum)
            ctx.fused = [dl, colsum]
        else:
            K.lovasz_fwd_bwd(buf, tgt, coef, counters, pixels, c, ldc, ignore_index, images, bins, ce_weight, partials, loss)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        n, c, h, w, ldc, ignore_index, images, bins, ce_weight = ctx.meta
        g = grad_out.detach().to(torch.float32).contiguous()
        if ctx.fused is not None:
            dl, colsum = ctx.fused
            ctx.fused = None                           # consumed
        else:                                          # a second backward through a retained graph: the same launch on the saved
            buf, tgt, coef, counters = ctx.saved_tensors                  # coefficient tables, so the same bits
            np_ = _load().udaseg_ce_partials()
            dl, parts, colsum = _OhemCrossEntropyFunction._grad_buffers(n, h, w, ldc, np_, buf.device)
            K.lovasz_fwd_bwd(buf, tgt, coef, counters, n * h * w, c, ldc, ignore_index, images, bins, ce_weight,
                             torch.empty(np_, device=buf.device, dtype=torch.float64),
                             torch.empty((), device=buf.device, dtype=torch.float32), dl, parts, colsum)
        K.scale_unless_one(dl, g, colsum)
        COLSUM_SIDE_TABLE.clear()
        COLSUM_SIDE_TABLE[dl.data_ptr()] = colsum
        return (dl.permute(0, 3, 1, 2)[:, :c],) + (None,) * 10


class LovaszSoftmaxLoss(nn.Module):
    """The Lovasz-softmax loss (Berman, Rannen Triki, Blaschko, CVPR 2018): the Lovasz extension of the per-class Jaccard loss,
    the direct surrogate of mean IoU.  ``[N,C,H,W]`` logits (C <= 32) and ``[N,H,W]`` integer targets, as ``CrossEntropyLoss``.

    For a group of pixels (the batch, or one image with ``per_image=True``) and a class ``c`` the error of a pixel is
    ``1 - p_c`` where the target is ``c`` and ``p_c`` elsewhere; the exact loss sorts the errors and weights them with the steps
    of the Jaccard loss.  Here nothing is sorted: the errors are counted into ``bins`` uniform bins per class (integer
    histograms), every pixel of a bin is treated as tied, and its weight is the average of the two orders "fg first" / "bg
    first" inside the bin, in closed form.  With ``L`` the exact loss and ``L_B`` this one, ``0 <= L - L_B <= sum(last_slack)
    <= 1 / bins`` (proved in DESIGN.md); ``L_B == L`` when no bin holds two pixels.  The weights are constants in the backward,
    as in the paper's implementation.

    * ``classes='present'`` averages over the classes that occur in the group's targets, ``'all'`` over all ``C``;
      ``per_image=True`` averages the per-image values over all ``N`` images.  A group without a valid pixel, or without a
      present class under 'present', contributes 0 and still counts as an image.
    * A pixel is valid as for ``CrossEntropyLoss`` (``target != ignore_index`` and ``0 <= target < C``); a valid pixel whose
      logits are not all finite is void as well.  Void pixels are in no table and their gradient is exactly 0.
    * ``ce_weight`` adds ``ce_weight *`` the mean cross entropy over the valid finite pixels in the same pass over the logits
      (the usual recipe is ``CE + Lovasz``: ``ce_weight=1.0``); with no valid pixel that term is NaN, ``CrossEntropyLoss``'s
      convention.

    After a call, all on the device and written by the loss's own launches (read them when convenient):

    * ``last_target_stats``: int64 ``[n_valid_finite, n_void, n_invalid, n_nonfinite]``;
    * ``last_present``: int32 ``[I, C]``, ``I = N`` with ``per_image`` and 1 without;
    * ``last_slack``: float64 ``[C]``; its sum bounds ``L - L_B`` of the value returned.

    Two calls give the same bits (integer atomics, fixed-order sums).  Under data parallelism each rank forms the loss of its
    own batch.
    """

    def __init__(self, classes='present', per_image=False, ignore_index=None, bins=1024, ce_weight=0.0):
        super().__init__()
        if classes not in ('present', 'all'):
            raise ValueError(f"LovaszSoftmaxLoss: classes must be 'present' or 'all', got {classes!r}")
        if isinstance(bins, bool) or int(bins) != bins or not 64 <= int(bins) <= 4096 or int(bins) & (int(bins) - 1):
            raise ValueError(f"LovaszSoftmaxLoss: bins must be a power of two in [64, 4096], got {bins!r}")
        ce_weight = float(ce_weight)
        if ce_weight != ce_weight or ce_weight in (float("inf"), float("-inf")):
            raise ValueError(f"LovaszSoftmaxLoss: ce_weight must be finite, got {ce_weight}")
        self.classes, self.per_image, self.bins, self.ce_weight = classes, bool(per_image), int(bins), ce_weight
        self.ignore_index = _check_ignore_index("LovaszSoftmaxLoss", ignore_index)
        self.last_target_stats = self.last_present = self.last_slack = None

    def extra_repr(self):
        return (f"classes={self.classes!r}, per_image={self.per_image}, ignore_index={self.ignore_index}, bins={self.bins}, "
                f"ce_weight={self.ce_weight}")

    def forward(self, input, target):
        if input.device.type != "cuda":
            raise RuntimeError("LovaszSoftmaxLoss: logits must live on the GPU (no CPU path in this build)")
        if input.dim() != 4 or target.dim() != 3 or input.shape[0] != target.shape[0] or input.shape[2:] != target.shape[1:]:
            raise ValueError(f"expected logits [N,C,H,W] and target [N,H,W]; got {tuple(input.shape)} and {tuple(target.shape)}")
        n, c, h, w = input.shape
        if c > 32:
            raise ValueError(f"LovaszSoftmaxLoss: at most 32 classes are supported by the HIP kernels, got {c}")
        if n * h * w >= 2 ** 31:
            raise ValueError(f"LovaszSoftmaxLoss: at most 2^31 - 1 pixels per call, got {n * h * w}")
        if target.dtype != torch.int64:
            target = target.long()
        dev = input.device
        images = n if self.per_image else 1
        tables = torch.zeros((images, c, 2, self.bins), device=dev, dtype=torch.int32)
        counters = torch.zeros(4, device=dev, dtype=torch.int64)
        present = torch.empty((images, c), device=dev, dtype=torch.int32)
        slack = torch.empty(c, device=dev, dtype=torch.float64)
        out = _LovaszSoftmaxFunction.apply(input, target.to(dev), self.ignore_index, images, self.bins, self.classes == 'all',
                                           self.ce_weight, tables, counters, present, slack)
        self.last_target_stats, self.last_present, self.last_slack = counters, present, slack
        return out


class _BCEPairFunction(torch.autograd.Function):
    """loss = w_a * mean(bce_with_logits(a, label_a)) + w_b * mean(bce_with_logits(b, label_b)); b optional."""

    @staticmethod
    def forward(ctx, a, label_a, w_a, b, label_b, w_b):
        a_c = a.detach().float().contiguous()
        loss = torch.empty((), device=a.device, dtype=torch.float32)
        K.bce_logits_fwd(a_c, label_a, w_a, loss, False)
        b_c = None
        if b is not None:
            b_c = b.detach().float().contiguous()
            K.bce_logits_fwd(b_c, label_b, w_b, loss, True)
        ctx.cfg = (label_a, w_a, label_b, w_b)
        ctx.save_for_backward(a_c, b_c)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        a_c, b_c = ctx.saved_tensors
        label_a, w_a, label_b, w_b = ctx.cfg
        g = grad_out.detach().float().contiguous()
        da = torch.empty_like(a_c)
        K.bce_logits_bwd(a_c, label_a, w_a, g, da, False)
        db = None
        if b_c is not None:
            db = torch.empty_like(b_c)
            K.bce_logits_bwd(b_c, label_b, w_b, g, db, False)
        return da, None, None, db, None, None


class _BCETargetFunction(torch.autograd.Function):
    """weight * mean(bce_with_logits(x, y)) with a per-sample target vector y."""

    @staticmethod
    def forward(ctx, x, y, weight):
        x_c = x.detach().float().contiguous()
        y_c = y.detach().float().contiguous()
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        K.bce_logits_target_fwd(x_c, y_c, weight, loss, False)
        ctx.save_for_backward(x_c, y_c)
        ctx.weight, ctx.shape = weight, x.shape
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x_c, y_c = ctx.saved_tensors
        dx = torch.empty_like(x_c)
        K.bce_logits_target_bwd(x_c, y_c, ctx.weight, grad_out.detach().float().contiguous(), dx, False)
        return dx.view(ctx.shape), None, None


class BCEWithLogitsLoss(nn.Module):
    """``nn.BCEWithLogitsLoss()`` as the reference constructs it (mean reduction, no weights; ``src/models/uda.py:85``)."""

    def forward(self, input, target):
        _need_gpu(input, "BCEWithLogitsLoss")
        if input.shape != target.shape:
            raise ValueError(f"Target size ({tuple(target.shape)}) must be the same as input size ({tuple(input.shape)})")
        return _BCETargetFunction.apply(input, target.to(input.device), 1.0)


class MulticlassDiceLoss(nn.Module):
    """``smp.losses.DiceLoss(mode='multiclass')`` with its defaults (from_logits, smooth 0, eps 1e-7, no ignore_index), the
    segmentation term of the reference's ``UDALoss`` (``src/models/uda.py:84``): Dice pooled over batch and pixels per
    class, classes absent from the batch's labels contribute 0, mean over all classes."""

    def __init__(self, smooth=0.0, eps=1e-7):
        super().__init__()
        self.smooth, self.eps = smooth, eps

    def forward(self, y_pred, y_true):
        y_true = _check_seg_pair("MulticlassDiceLoss", y_pred, y_true)
        return _SegLossFunction.apply(y_pred, y_true, None, 0.0, 0.0, True, float(self.smooth), 0.0, 1.0, float(self.eps), True)


def _need_gpu(t, who):
    if t.device.type != "cuda":
        raise RuntimeError(f"{who}: predictions must live on the GPU (no CPU path in this build)")


class AdversarialLoss:
    def __init__(self, lambda_adv=0.001):
        """Adversarial loss for domain adaptation.  lambda_adv: weight of the generator term (default 0.001)."""
        self.lambda_adv = lambda_adv

    def discriminator_loss(self, source_pred, target_pred):
        """(BCEWithLogits(source_pred, 1) + BCEWithLogits(target_pred, 0)) / 2"""
        _need_gpu(source_pred, "AdversarialLoss.discriminator_loss")
        return _BCEPairFunction.apply(source_pred, 1.0, 0.5, target_pred, 0.0, 0.5)

    def generator_loss(self, target_pred):
        """lambda_adv * BCEWithLogits(target_pred, 1)"""
        _need_gpu(target_pred, "AdversarialLoss.generator_loss")
        return _BCEPairFunction.apply(target_pred, 1.0, float(self.lambda_adv), None, 0.0, 0.0)


# ------------------------------------------------------------------------------------------ Dice / focal / consistency
def _check_seg_pair(who, logits, target):
    _need_gpu(logits, who)
    if logits.dim() != 4:
        raise ValueError(f"{who}: expected predictions [B,C,H,W], got {tuple(logits.shape)}")
    if logits.shape[1] > 32:
        raise ValueError(f"{who}: at most 32 classes are supported by the HIP kernels, got {logits.shape[1]}")
    if target.dim() == 4:
        # the reference also takes one-hot [B,C,H,W] targets; the kernels work from class indices
        target = target.argmax(dim=1)
    if target.dim() != 3 or target.shape[0] != logits.shape[0] or target.shape[1:] != logits.shape[2:]:
        raise ValueError(f"{who}: targets {tuple(target.shape)} do not match predictions {tuple(logits.shape)}")
    return target.long().contiguous()


def _check_ignore_index(who, ignore_index):
    if ignore_index is None:
        return None
    if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index or not -2 ** 63 <= int(ignore_index) < 2 ** 63:
        raise ValueError(f"{who}: ignore_index must be None or an int64, got {ignore_index!r}")
    return int(ignore_index)


class _SegLossFunction(torch.autograd.Function):
    """loss = focal_w * focal(logits, target) + dice_w * dice(logits, target); either weight may be 0 (term skipped)."""

    @staticmethod
    def forward(ctx, logits, target, class_weights, alpha, gamma, mean, smooth, focal_w, dice_w, dice_eps=1e-7,
                dice_pooled=False, ignore_index=None):
        n, c, h, w = logits.shape
        buf, ldc = padded_nhwc(logits.detach())
        dev = logits.device
        loss = torch.zeros((), device=dev, dtype=torch.float32)
        coef = None
        if focal_w != 0.0:
            parts = torch.empty(K.seg_partials(), device=dev, dtype=torch.float64)
            K.focal_fwd(buf, target, class_weights, alpha, gamma, n * h * w, c, ldc, mean, parts, loss, ignore_index=ignore_index)
            if focal_w != 1.0:
                loss.mul_(focal_w)
        if dice_w != 0.0:
            sums = torch.zeros(n * 3 * c, device=dev, dtype=torch.float64)
            coef = torch.empty(n * 2 * c, device=dev, dtype=torch.float32)
            dloss = torch.empty((), device=dev, dtype=torch.float32)
            K.dice_fwd(buf, target, n, h * w, c, ldc, smooth, sums, coef, dloss, dice_eps, dice_pooled, ignore_index=ignore_index)
            loss.add_(dloss, alpha=dice_w)
        ctx.save_for_backward(buf, target, class_weights, coef)
        ctx.cfg = (n, c, h, w, ldc, alpha, gamma, mean, focal_w, dice_w)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        buf, target, class_weights, coef = ctx.saved_tensors
        n, c, h, w, ldc, alpha, gamma, mean, focal_w, dice_w = ctx.cfg
        g = grad_out.detach().float().contiguous()
        dl = torch.empty((n, h, w, ldc), device=buf.device, dtype=torch.float32)
        wrote = False
        if focal_w != 0.0:
            K.focal_bwd(buf, target, class_weights, alpha, gamma, g, focal_w / (n * h * w) if mean else focal_w, n * h * w, c,
                        ldc, dl, False, ignore_index=ctx.ignore_index)
            wrote = True
        if dice_w != 0.0:
            K.dice_bwd(buf, target, coef, g, dice_w, n, h * w, c, ldc, dl, wrote, ignore_index=ctx.ignore_index)
        return (dl.permute(0, 3, 1, 2)[:, :c],) + (None,) * 11


class DiceLoss(nn.Module):
    """1 - mean over (image, class) of the soft Dice coefficient of softmax(predictions) against the labels.

    ``ignore_index`` (opt-in, default None = as before): pixels labelled ``ignore_index`` or outside ``[0, C)`` are left out of the
    intersection, the probability sum and the label count of every image and class, and get a gradient of exactly 0."""

    def __init__(self, smooth=1.0, ignore_index=None):
        super().__init__()
        self.smooth = smooth
        self.ignore_index = _check_ignore_index("DiceLoss", ignore_index)

    def forward(self, predictions, targets):
        targets = _check_seg_pair("DiceLoss", predictions, targets)
        return _SegLossFunction.apply(predictions, targets, None, 0.0, 0.0, True, float(self.smooth), 0.0, 1.0, 1e-7, False,
                                      self.ignore_index)


class WeightedSegmentationLoss(nn.Module):
    """domain_weight * (focal-modulated class-weighted cross entropy + Dice).

    ``ignore_index`` (opt-in, default None = as before): at pixels labelled ``ignore_index`` or outside ``[0, C)`` the cross
    entropy, hence the focal term, is 0 (``F.cross_entropy(..., ignore_index=...)`` in the reference's line; 'mean' still divides
    by N*H*W), the class weight of such a label is never read, and the Dice term leaves them out."""

    def __init__(self, num_classes: int, class_weights: Optional[torch.Tensor] = None, alpha: float = 0.25,
                 gamma: float = 2.0, reduction: str = 'mean', ignore_index: Optional[int] = None):
        super().__init__()
        self.ignore_index = _check_ignore_index("WeightedSegmentationLoss", ignore_index)
        self.num_classes = num_classes
        self.register_buffer('class_weights', torch.ones(num_classes) if class_weights is None else class_weights)
        self.alpha = alpha
        self.gamma = gamma
        self.reduction = reduction
        self.dice_loss = DiceLoss(ignore_index=self.ignore_index)

    def _weights_on(self, device):
        return self.class_weights.to(device=device, dtype=torch.float32).contiguous()

    def focal_loss(self, inputs, targets):
        targets = _check_seg_pair("WeightedSegmentationLoss.focal_loss", inputs, targets)
        return _SegLossFunction.apply(inputs, targets, self._weights_on(inputs.device), float(self.alpha), float(self.gamma),
                                      self.reduction == 'mean', 1.0, 1.0, 0.0, 1e-7, False, self.ignore_index)

    def forward(self, inputs, targets, domain_weight: float = 1.0):
        if inputs.dim() == 4 and inputs.shape[1] != self.num_classes:
            raise ValueError(f"WeightedSegmentationLoss: {inputs.shape[1]} channels for {self.num_classes} classes")
        targets = _check_seg_pair("WeightedSegmentationLoss", inputs, targets)
        both = _SegLossFunction.apply(inputs, targets, self._weights_on(inputs.device), float(self.alpha), float(self.gamma),
                                      self.reduction == 'mean', float(self.dice_loss.smooth), 1.0, 1.0, 1e-7, False, self.ignore_index)
        return domain_weight * both


def calculate_class_weights(dataset, num_classes: int, method: str = 'effective_samples') -> torch.Tensor:
    """Class weights from pixel counts over ``dataset`` (items ``(image, mask)``): 'effective_samples' uses
    (1-beta)/(1-beta^n) with beta=0.9999, anything else 1/n; normalised to sum to num_classes."""
    counts = torch.zeros(num_classes)
    for _, mask in dataset:
        m = torch.as_tensor(mask).reshape(-1).long()
        m = m[(m >= 0) & (m < num_classes)]
        counts += torch.bincount(m, minlength=num_classes).to(counts.dtype)
    counts = counts.clamp(min=1.0)
    if method == 'effective_samples':
        beta = 0.9999
        weights = (1.0 - beta) / (1.0 - torch.pow(beta, counts))
    else:
        weights = 1.0 / counts
    return weights / weights.sum() * num_classes


class _ConsistencyFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred1, pred2, temperature):
        n, c, h, w = pred1.shape
        z1, ldc = padded_nhwc(pred1.detach())
        z2, _ = padded_nhwc(pred2.detach())
        dev = pred1.device
        parts = torch.empty(K.seg_partials(), device=dev, dtype=torch.float64)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        K.consistency_fwd(z1, z2, temperature, n, n * h * w, c, ldc, parts, loss)
        ctx.save_for_backward(z1, z2)
        ctx.cfg = (n, c, h, w, ldc, temperature)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        z1, z2 = ctx.saved_tensors
        n, c, h, w, ldc, temperature = ctx.cfg
        g = grad_out.detach().float().contiguous()
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d1 = torch.empty((n, h, w, ldc), device=z1.device, dtype=torch.float32) if need1 else None
        d2 = torch.empty((n, h, w, ldc), device=z1.device, dtype=torch.float32) if need2 else None
        if need1 or need2:
            K.consistency_bwd(z1, z2, temperature, g, 1.0, n, n * h * w, c, ldc, d1, d2)
        return (d1.permute(0, 3, 1, 2)[:, :c] if need1 else None, d2.permute(0, 3, 1, 2)[:, :c] if need2 else None, None)


class ConsistencyLoss(nn.Module):
    """Symmetric KL between the temperature-softened class distributions of two predictions of the same image."""

    def __init__(self, temperature=0.5):
        super().__init__()
        self.temperature = temperature

    def forward(self, pred1, pred2):
        _need_gpu(pred1, "ConsistencyLoss")
        if pred1.dim() != 4 or pred1.shape != pred2.shape:
            raise ValueError(f"ConsistencyLoss: expected two [B,C,H,W] predictions, got {tuple(pred1.shape)} and {tuple(pred2.shape)}")
        if pred1.shape[1] > 32:
            raise ValueError("ConsistencyLoss: at most 32 classes are supported by the HIP kernels")
        return _ConsistencyFunction.apply(pred1, pred2, float(self.temperature))

    def get_similarity_matrix(self, pred1, pred2):
        """Per-pixel cosine similarity of the two softmax distributions, [B,H,W] (visualisation helper, not on the hot
        path: plain torch ops)."""
        return torch.nn.functional.cosine_similarity(torch.softmax(pred1, dim=1), torch.softmax(pred2, dim=1), dim=1)


class _EntropyFunction(torch.autograd.Function):
    """Entropy / maximum-squares loss of a prediction (csrc/advent.hip).  As ``_CrossEntropyFunction``'s fused branch: when the
    input needs a gradient it is made in the forward's pass over the logits; backward only scales it if it has to.  A second
    backward through a retained graph re-runs the entry point."""

    @staticmethod
    def forward(ctx, logits, kind):
        n, c, h, w = logits.shape
        buf, ldc = padded_nhwc(logits.detach())
        dev = logits.device
        loss = torch.empty((), device=dev, dtype=torch.float32)
        parts = torch.empty(K.seg_partials(), device=dev, dtype=torch.float64)
        dl = torch.empty((n, h, w, ldc), device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        K.entropy_loss(buf, n * h * w, c, ldc, kind, parts, loss, dl)
        ctx.meta, ctx.fused = (n, c, h, w, ldc, kind), dl
        ctx.save_for_backward(buf)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        n, c, h, w, ldc, kind = ctx.meta
        g = grad_out.detach().to(torch.float32).contiguous()
        dl, ctx.fused = ctx.fused, None                # consumed: scaled in place below
        if dl is None:
            buf, = ctx.saved_tensors
            dl = torch.empty((n, h, w, ldc), device=buf.device, dtype=torch.float32)
            K.entropy_loss(buf, n * h * w, c, ldc, kind, torch.empty(K.seg_partials(), device=buf.device, dtype=torch.float64),
                           torch.empty((), device=buf.device, dtype=torch.float32), dl)
        K.scale_unless_one(dl, g)
        return dl.permute(0, 3, 1, 2)[:, :c], None


class EntropyLoss(nn.Module):
    """The direct part of output-space adaptation: a loss of the prediction alone, no labels (target frames).

    ``kind='entropy'`` (MinEnt, Vu et al., CVPR 2019): the mean over the pixels of the normalised entropy
    ``-sum_c p_c log p_c / log C`` in ``[0, 1]``.  ``kind='max_squares'`` (Chen et al., ICCV 2019): ``-mean_pixels sum_c p_c^2 / 2``,
    whose gradient does not vanish on the confident pixels the way the entropy's does.  A class whose probability is 0 contributes
    exactly 0 to the loss and to the gradient.  ``forward(logits [B,C,H,W]) -> scalar``, ``2 <= C <= 32``."""

    def __init__(self, kind="entropy"):
        super().__init__()
        if kind not in K.ENTROPY_KINDS:
            raise ValueError(f"EntropyLoss: kind must be one of {sorted(K.ENTROPY_KINDS)}, got {kind!r}")
        self.kind = kind

    def extra_repr(self):
        return f"kind={self.kind!r}"

    def forward(self, logits):
        _check_prediction("EntropyLoss", logits)
        return _EntropyFunction.apply(logits, self.kind)


class _SoftCrossEntropyFunction(torch.autograd.Function):
    """Soft-target loss of student logits against a teacher distribution (csrc/distill.hip), shaped like
    ``_CrossEntropyOptFunction``: for 'weighted_mean' one launch over the weights alone makes D first; then ONE pass reads both
    rows and, when the logits need a gradient, writes it already scaled with the head's bias gradient (column sums); backward
    only scales it if it has to.  A second backward through a retained graph re-runs the entry point."""

    @staticmethod
    def forward(ctx, logits, tbuf, ldt, probs, wpx, wimg, cfg, stats):
        n, c, h, w = logits.shape
        buf, ldc = padded_nhwc(logits.detach())
        dev = logits.device
        denom = None
        if cfg["reduction"] == 'weighted_mean':
            denom = torch.empty(1, device=dev, dtype=torch.float64)
            K.pixel_weight_sum(wpx, wimg, n, h * w, torch.empty(3 * K.seg_partials(), device=dev, dtype=torch.float64), denom,
                               torch.empty(2, device=dev, dtype=torch.int64))
        ctx.meta = (n, c, h, w, ldc, ldt, probs, cfg)
        ctx.save_for_backward(buf, tbuf, wpx, wimg, denom)
        ctx.fused = None
        loss = torch.empty((), device=dev, dtype=torch.float32)
        if ctx.needs_input_grad[0]:
            ctx.fused = _SoftCrossEntropyFunction._run(ctx.meta, buf, tbuf, wpx, wimg, denom, loss, stats, True)
        else:
            _SoftCrossEntropyFunction._run(ctx.meta, buf, tbuf, wpx, wimg, denom, loss, stats, False)
        return loss

    @staticmethod
    def _run(meta, buf, tbuf, wpx, wimg, denom, loss, stats, grad):
        n, c, h, w, ldc, ldt, probs, cfg = meta
        dev = buf.device
        partials = torch.empty(K.seg_partials(), device=dev, dtype=torch.float64)
        dl = parts = colsum = None
        if grad:
            dl = torch.empty((n, h, w, ldc), device=dev, dtype=torch.float32)
            parts = torch.empty(K.seg_partials() * ldc, device=dev, dtype=torch.float32)
            colsum = torch.empty(ldc, device=dev, dtype=torch.float32)
        K.soft_ce_fwd_bwd(buf, tbuf, wpx, wimg, n, h * w, c, ldc, ldt, probs, cfg["kind"], cfg["inv_temp"], cfg["alpha"], cfg["beta"],
                          cfg["log_floor"], cfg["reduction"] == 'mean', denom, partials, loss, dl, parts, colsum, stats)
        return [dl, colsum] if grad else None

    @staticmethod
    def backward(ctx, grad_out):
        n, c, h, w = ctx.meta[:4]
        g = grad_out.detach().to(torch.float32).contiguous()
        fused, ctx.fused = ctx.fused, None             # consumed: scaled in place below
        if fused is None:
            buf, tbuf, wpx, wimg, denom = ctx.saved_tensors
            fused = _SoftCrossEntropyFunction._run(ctx.meta, buf, tbuf, wpx, wimg, denom,
                                                   torch.empty((), device=buf.device, dtype=torch.float32), None, True)
        dl, colsum = fused
        K.scale_unless_one(dl, g, colsum)
        COLSUM_SIDE_TABLE.clear()
        COLSUM_SIDE_TABLE[dl.data_ptr()] = colsum
        return (dl.permute(0, 3, 1, 2)[:, :c],) + (None,) * 7


class SoftCrossEntropyLoss(nn.Module):
    """A loss between student logits and a teacher DISTRIBUTION, with per-pixel and per-image weights: distillation.

    ``forward(logits [N,C,H,W], teacher [N,C,H,W], probs=False, pixel_weight=None [N,H,W], image_weight=None [N]) -> scalar``,
    ``2 <= C <= 32``.  The teacher is logits, softened as ``softmax(teacher / teacher_temperature)`` (Hinton et al. 2015; the
    student is not softened and no ``T^2`` is applied), or with ``probs=True`` probabilities taken as they are (what
    ``proto.rectify`` and ``predict_large(..., return_probs=True)`` produce).  It never receives a gradient, and a teacher tensor
    that requires one raises.  With ``q`` the teacher's distribution, ``p`` the student's and ``Q = sum_c q_c``:

    * ``kind='ce'``: ``-sum_c q_c log p_c``;  ``kind='kl'``: ``sum_c q_c (log q_c - log p_c)`` -- the same gradient ``Q p - q``;
    * ``kind='symmetric'`` (Wang et al., ICCV 2019): ``alpha * ce + beta * sum_c p_c g_c``, ``g_c = -max(log q_c, log_floor)``
      (the paper's ``A = -4``; ``-log_floor`` where ``q_c == 0``).

    Pixel ``p`` of image ``i`` weighs ``w = pixel_weight[p] * image_weight[i]`` (missing: 1).  A pixel is *void* -- loss and
    gradient exactly 0 -- when ``w`` is 0, negative or not finite, when its teacher row holds a non-finite value (the NaN rows of
    ``proto.rectify``), or, with ``probs``, a value outside ``[0, 1]`` or only zeros.  ``reduction``: 'mean' divides the weighted
    sum by ``N*H*W`` (DACS's and DAFormer's ``mean(q_i * ce_p)``), 'sum' by nothing, 'weighted_mean' by the sum of the weights
    that do not void their pixel (all void: NaN, as ``CrossEntropyLoss`` over void labels only).  ``last_stats``: device int64
    ``[counted, void by a zero weight, void otherwise]`` of the last call, written by the loss's own launch: read it when convenient.
    """

    REDUCTIONS = ('mean', 'sum', 'weighted_mean')

    def __init__(self, kind="ce", teacher_temperature=1.0, alpha=1.0, beta=1.0, log_floor=-4.0, reduction='mean'):
        super().__init__()
        import math
        if kind not in K.SOFT_CE_KINDS:
            raise ValueError(f"SoftCrossEntropyLoss: kind must be one of {sorted(K.SOFT_CE_KINDS)}, got {kind!r}")
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"SoftCrossEntropyLoss: reduction must be one of {self.REDUCTIONS}, got {reduction!r}")
        t = float(teacher_temperature)
        if not (t > 0.0 and math.isfinite(t)):
            raise ValueError(f"SoftCrossEntropyLoss: teacher_temperature must be positive and finite, got {teacher_temperature}")
        if not (math.isfinite(float(alpha)) and math.isfinite(float(beta))):
            raise ValueError(f"SoftCrossEntropyLoss: alpha and beta must be finite, got {alpha} and {beta}")
        if not (float(log_floor) < 0.0 and math.isfinite(float(log_floor))):
            raise ValueError(f"SoftCrossEntropyLoss: log_floor must be negative and finite, got {log_floor}")
        self.kind, self.reduction = kind, reduction
        self.teacher_temperature, self.alpha, self.beta, self.log_floor = t, float(alpha), float(beta), float(log_floor)
        self.last_stats = None

    def extra_repr(self):
        return (f"kind={self.kind!r}, teacher_temperature={self.teacher_temperature}, alpha={self.alpha}, beta={self.beta}, "
                f"log_floor={self.log_floor}, reduction={self.reduction!r}")

    def forward(self, logits, teacher, probs=False, pixel_weight=None, image_weight=None):
        _check_prediction("SoftCrossEntropyLoss", logits)
        n, c, h, w = logits.shape
        if not torch.is_tensor(teacher) or tuple(teacher.shape) != (n, c, h, w):
            raise ValueError(f"SoftCrossEntropyLoss: teacher must be a [{n},{c},{h},{w}] tensor like the logits, got "
                             f"{tuple(getattr(teacher, 'shape', ()))}")
        if teacher.requires_grad:
            raise ValueError("SoftCrossEntropyLoss: the teacher never receives a gradient; pass teacher.detach()")
        for name, t, shape in (("pixel_weight", pixel_weight, (n, h, w)), ("image_weight", image_weight, (n,))):
            if t is None:
                continue
            if not torch.is_tensor(t) or tuple(t.shape) != shape or not t.is_floating_point():
                raise ValueError(f"SoftCrossEntropyLoss: {name} must be a floating-point tensor of shape {shape}, got "
                                 f"{tuple(getattr(t, 'shape', ()))}")
            if t.requires_grad:
                raise ValueError(f"SoftCrossEntropyLoss: {name} never receives a gradient; pass {name}.detach()")
        for name, t in (("teacher", teacher), ("pixel_weight", pixel_weight), ("image_weight", image_weight)):
            if t is not None and t.device != logits.device:
                raise RuntimeError(f"SoftCrossEntropyLoss: {name} must live on the logits' GPU (no CPU path in this build)")
        tbuf, ldt = padded_nhwc(teacher)
        dev = logits.device
        wpx = None if pixel_weight is None else pixel_weight.to(torch.float32).contiguous()
        wimg = None if image_weight is None else image_weight.to(torch.float32).contiguous()
        cfg = dict(kind=self.kind, inv_temp=1.0 / self.teacher_temperature, alpha=self.alpha, beta=self.beta,
                   log_floor=self.log_floor, reduction=self.reduction)
        stats = torch.zeros(3, device=dev, dtype=torch.int64)
        out = _SoftCrossEntropyFunction.apply(logits, tbuf, ldt, bool(probs), wpx, wimg, cfg, stats)
        self.last_stats = stats
        return out


def _check_prediction(who, logits):
    """A prediction the output-space kernels take: on the GPU, [B,C,H,W], 2 <= C <= 32 (log C divides)."""
    if logits.dim() != 4:
        raise ValueError(f"{who}: expected predictions [B,C,H,W], got {tuple(logits.shape)}")
    if not 2 <= logits.shape[1] <= 32:
        raise ValueError(f"{who}: 2 to 32 classes are supported by the HIP kernels, got {logits.shape[1]}")
    _need_gpu(logits, who)


class FineTuningLoss(nn.Module):
    """Phase-3 objective: ramped consistency + ramped domain confusion (+ Dice on labelled samples when given).

    As upstream, ``domain_weight`` enters twice: as ``AdversarialLoss(lambda_adv=domain_weight)`` and again as the
    multiplier of that term."""

    def __init__(self, consistency_weight: float = 1.0, domain_weight: float = 0.1, supervised_weight: float = 0.1,
                 rampup_length: int = 40, temperature: float = 0.5):
        super().__init__()
        self.consistency_loss = ConsistencyLoss(temperature=temperature)
        self.domain_loss = AdversarialLoss(lambda_adv=domain_weight)
        self.supervised_loss = DiceLoss()
        self.consistency_weight = consistency_weight
        self.domain_weight = domain_weight
        self.supervised_weight = supervised_weight
        self.rampup_length = rampup_length

    def rampup(self, epoch: int) -> float:
        """Linear 0 -> 1 over the first ``rampup_length`` epochs, 1 afterwards."""
        return 1.0 if epoch >= self.rampup_length else float(epoch) / self.rampup_length

    def forward(self, pred1, pred2, domain_pred, epoch: int, supervised_pred=None,
                supervised_target=None) -> Dict[str, torch.Tensor]:
        ramp = self.rampup(epoch)
        consistency = self.consistency_loss(pred1, pred2)
        domain_confusion = self.domain_loss.generator_loss(domain_pred)
        total = consistency * (self.consistency_weight * ramp) + domain_confusion * (self.domain_weight * ramp)
        supervised = torch.tensor(0.0, device=pred1.device)
        if supervised_pred is not None and supervised_target is not None:
            supervised = self.supervised_loss(supervised_pred, supervised_target)
            total = total + supervised * self.supervised_weight
        return {'total': total, 'consistency': consistency.detach(), 'domain_confusion': domain_confusion.detach(),
                'supervised': supervised.detach(), 'rampup_weight': torch.tensor(ramp)}
