"""Prototype-rectified pseudo-labels on the decoder's features: the feature-space check of the self-training stack.  An
EXTENSION: the reference has no counterpart.  The method is ProDA's (Zhang et al. 2021): ``pseudo.py``, ``mix.py``
and ``teacher.py`` judge a target pixel by the teacher's softmax alone, and a teacher that is confidently wrong under domain
shift passes every confidence threshold.  Here one prototype per class is kept in the space of the 16-channel full-resolution
decoder output (``Unet.forward_parts(x, ("logits", "decoder"))`` returns it beside the logits in one pass), every pixel's class
probabilities are re-weighted by how close its feature lies to each prototype, and ``pseudo.py``'s table, thresholds and labels
then work on the re-weighted probabilities (``probs=True``).

With torch this is an ``index_add_`` per batch, a ``[pixels, C, D]`` broadcast for the distances, two softmaxes and a
normalisation.  Here: ONE streaming HIP pass accumulates per-class float64 sums (``udaseg_proto_accumulate``), one small block
updates the prototypes and the temperature (``udaseg_proto_update``), ONE streaming pass writes the rectified probabilities
(``udaseg_proto_rectify``); nothing is read back.

The contract (include/udaseg.h, INTEGRATION.md "Prototype rectification"; ``update_mirror`` / ``rectify_mirror`` state it in numpy)
    accumulate: a pixel with label ``c < C`` and finite features adds its feature to ``sums[c]``, its squared norm to ``sq[c]``
    and 1 to ``counts[c]``, all in float64; other labels are counted in ``counts[C]``, non-finite features in ``counts[C + 1]``.
    update: for a class with ``n = counts[c] >= min_pixels``: ``mean = sums[c] / n``, ``s = max(sq[c] / n - |mean|^2, 0)`` (the
    mean squared distance of the batch's features to their mean); first sight copies ``mean`` and ``s``, later updates are
    the EMA ``momentum * old + (1 - momentum) * new``; float64, no fused multiply-add, bit for bit ``update_mirror``.
    ``tau="auto"``: ``tau = tau_scale *`` the mean spread of the seen classes (the distances are then measured in units of the
    classes' own scatter); a float ``tau`` is fixed.  The kernels carry ``inv_tau = float32(1 / tau)``, 0 while no class is seen.
    rectify, per pixel in fp32: ``p`` = softmax of the logits (or the given probabilities), ``d_c = |f - float32(proto_c)|^2``,
    ``u_c = exp(-(d_c - min_seen d) * inv_tau)`` for a seen class, 0 for an unseen one (1 for all while none is seen),
    ``out = p * u / sum(p * u)``.  A row is NaN when a feature or a score is not finite, a probability lies outside ``[0, 1]``
    or the sum is zero or not finite: ``pseudo.py``'s ``probs=True`` contract labels that pixel void and counts it.

Deviations from ProDA: the weights are ``exp(-(d - d_min) / tau)`` renormalised against ``p`` rather than a softmax over
``-d / tau`` multiplied in (the same numbers: the softmax's denominator cancels in the renormalisation); squared Euclidean
distance in the decoder's 16 channels, not in a 256-channel ASPP output; the prototypes follow the RAW winner of the current
teacher in one streaming EMA per batch (ProDA's initialisation rule applied online) and there is no second-stage distillation.

The prototypes also SHAPE the features (ProDA's target structure learning; ProCA, SePiCo: csrc/proto_contrast.hip, INTEGRATION.md
"Prototype contrast and structure learning"): ``assign`` is a pixel's soft assignment to the seen prototypes, the softmax of
``-(d_c - d*) * inv_tau`` over them (``udaseg_proto_assign``; ``assign_mirror``), and ``PrototypeContrastLoss`` the cross entropy of
that assignment against a label mask or another distribution, differentiated with respect to the FEATURES in the same pass
(``udaseg_proto_contrast_fwd_bwd``; ``contrast_mirror``); the prototypes receive no gradient.  ``structure.StructureTrainer`` trains
with both.

Use, in place of ``teacher.OnlineLabeler`` in the mean-teacher recipe::

    labeler = proto.PrototypeLabeler(mt, num_classes=23, portion=0.2, cap=0.9, halve_every=100, rectify_after=200)
    labeler.init_from(source_loader_u8)            # optional: (frames, masks) batches -> source-initialised prototypes
    mixed = mix.MixedLoader(source_loader_u8, labeler.loader(target_loader_u8), num_classes=23, generator=g)
"""
import numpy as np
import torch

from . import _args as A
from . import kernels as K
from . import pseudo, teacher

DECODER_DIM = 16


def _check_dim(dim):
    if A.int_in("proto", "dim", dim, 4, 64) % 4:
        raise ValueError(f"proto: dim must be a multiple of 4, got {dim}")
    return int(dim)


def _check_momentum(momentum):
    return A.number("proto", "momentum", momentum, 0.0, 1.0)


def _check_min_pixels(min_pixels):
    return A.int_in("proto", "min_pixels", min_pixels, 1)


def _check_tau(tau, tau_scale):
    """-> (fixed tau or None for "auto", tau_scale)."""
    tau_scale = A.number("proto", "tau_scale", tau_scale, 0.0, lo_open=True)
    return (None if tau == "auto" else A.number("proto", "tau ('auto' or a float)", tau, 0.0, lo_open=True)), tau_scale


# ---------------------------------------------------------------------------------------------------------- host mirrors
def update_mirror(sums, sq, counts, proto, spread, seen, momentum=0.999, min_pixels=16, tau_scale=1.0, inv_tau=0.0):
    """``udaseg_proto_update`` on the host in numpy float64 / int64, bit for bit (every product, quotient and sum is one IEEE
    operation, in the kernel's order).  ``sums [C, D]``, ``sq [C]``, ``counts [C + 2]``: the accumulators; ``proto [C, D]``,
    ``spread [C]``, ``seen [C]``: the state before.  Returns ``(proto, spread, seen int32, last_counts int64, inv_tau float32)``;
    with ``tau_scale <= 0`` the given ``inv_tau`` comes back.  Needs no GPU."""
    sums = np.array(sums, dtype=np.float64)
    sq = np.array(sq, dtype=np.float64)
    counts = np.array(counts, dtype=np.int64)
    proto = np.array(proto, dtype=np.float64)
    spread = np.array(spread, dtype=np.float64)
    seen = np.array(seen, dtype=np.int32)
    if sums.ndim != 2 or proto.shape != sums.shape:
        raise ValueError(f"sums and proto must be [C, D] tables of one shape, got {sums.shape} and {proto.shape}")
    C, D = sums.shape
    if sq.shape != (C,) or spread.shape != (C,) or seen.shape != (C,) or counts.shape != (C + 2,):
        raise ValueError(f"sq, spread, seen must be [{C}] and counts [{C + 2}]")
    mom = np.float64(_check_momentum(momentum))
    min_pixels = _check_min_pixels(min_pixels)
    om = np.float64(1.0) - mom
    zero = np.float64(0.0)
    with np.errstate(all="ignore"):
        for c in range(C):
            n = int(counts[c])
            if n < min_pixels:
                continue
            dn = np.float64(n)
            mean = sums[c] / dn
            msq = zero
            for j in range(D):
                msq = msq + mean[j] * mean[j]
            diff = sq[c] / dn - msq
            s = diff if diff > zero else zero
            if not seen[c]:
                proto[c] = mean
                spread[c] = s
                seen[c] = 1
            else:
                proto[c] = mom * proto[c] + om * mean
                spread[c] = mom * spread[c] + om * s
        out_inv = np.float32(inv_tau)
        if float(tau_scale) > 0.0:
            tot, ns = zero, 0
            for c in range(C):
                if seen[c]:
                    tot = tot + spread[c]
                    ns += 1
            t = np.float64(tau_scale) * (tot / np.float64(ns))
            out_inv = np.float32(np.float64(1.0) / t) if np.isfinite(t) and t > zero else np.float32(0.0)
    return proto, spread, seen, counts.copy(), out_inv


def rectify_mirror(features, scores, proto, seen, inv_tau, probs=False):
    """The rectification formula in numpy float64 (what ``udaseg_proto_rectify`` evaluates in fp32).  ``features [P, D]``,
    ``scores [P, C]`` (logits, or probabilities with ``probs``), ``proto [C, D]`` (rounded to float32 first, as the kernel stages
    it), ``seen [C]``, ``inv_tau``: a number.  Returns ``[P, C]`` float64 with NaN rows where the contract says so.  Needs no GPU."""
    f = np.asarray(features, dtype=np.float64)
    z = np.asarray(scores, dtype=np.float64)
    pr = np.asarray(proto, dtype=np.float64).astype(np.float32).astype(np.float64)
    seen = np.asarray(seen).astype(bool)
    if f.ndim != 2 or z.ndim != 2 or pr.ndim != 2 or f.shape[0] != z.shape[0] or pr.shape != (z.shape[1], f.shape[1]):
        raise ValueError(f"features [P, D], scores [P, C], proto [C, D] expected, got {f.shape}, {z.shape}, {pr.shape}")
    if seen.shape != (z.shape[1],):
        raise ValueError(f"seen must be [{z.shape[1]}], got {seen.shape}")
    it = np.float64(inv_tau)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(f).all(axis=1) | ~np.isfinite(z).all(axis=1)
        if probs:
            p = z
            bad |= ~((z >= 0.0) & (z <= 1.0)).all(axis=1)
        else:
            e = np.exp(z - z.max(axis=1, keepdims=True))
            p = e / e.sum(axis=1, keepdims=True)
        if seen.any():
            d = ((f[:, None, :] - pr[None, :, :]) ** 2).sum(axis=2)
            dmin = d[:, seen].min(axis=1, keepdims=True)
            u = np.where(seen[None, :], np.exp(-(d - dmin) * it), 0.0)
            r = np.where(seen[None, :], p * u, 0.0)
        else:
            r = p.copy()
        R = r.sum(axis=1, keepdims=True)
        bad |= ~(np.isfinite(R[:, 0]) & (R[:, 0] > 0.0))
        out = r / R
    out[bad] = np.nan
    return out


def _mirror_operands(features, proto, seen):
    f = np.asarray(features, dtype=np.float64)
    pr = np.asarray(proto, dtype=np.float64).astype(np.float32).astype(np.float64)
    seen = np.asarray(seen).astype(bool)
    if f.ndim != 2 or pr.ndim != 2 or pr.shape[1] != f.shape[1]:
        raise ValueError(f"features [P, D], proto [C, D] expected, got {f.shape}, {pr.shape}")
    if seen.shape != (pr.shape[0],):
        raise ValueError(f"seen must be [{pr.shape[0]}], got {seen.shape}")
    return f, pr, seen


def _assignment(f, pr, seen, it):
    """(a [P, C], L [P], s [P, C]) of the contract over the seen classes (at least one); unseen columns: a = 0, s = 0."""
    d = ((f[:, None, :] - pr[None, :, :]) ** 2).sum(axis=2)
    dmin = d[:, seen].min(axis=1, keepdims=True)
    a = np.where(seen[None, :], -(d - dmin) * it, 0.0)
    L = np.log(np.where(seen[None, :], np.exp(a), 0.0).sum(axis=1))
    return a, L, np.where(seen[None, :], np.exp(a - L[:, None]), 0.0)


def assign_mirror(features, proto, seen, inv_tau):
    """``udaseg_proto_assign``'s contract in numpy float64: the softmax of ``-(d_c - d*) * inv_tau`` over the seen classes, 0 for
    an unseen one, ``1 / C`` everywhere while none is seen, NaN rows for non-finite features.  ``features [P, D]``, ``proto
    [C, D]`` (rounded to float32 first, as the kernel stages it), ``seen [C]``.  Returns ``[P, C]`` float64.  Needs no GPU."""
    f, pr, seen = _mirror_operands(features, proto, seen)
    with np.errstate(all="ignore"):
        if seen.any():
            out = _assignment(f, pr, seen, np.float64(inv_tau))[2]
        else:
            out = np.full((f.shape[0], pr.shape[0]), 1.0 / pr.shape[0])
        out[~np.isfinite(f).all(axis=1)] = np.nan
    return out


CONTRAST_REDUCTIONS = ("mean", "sum", "weighted_mean")


def contrast_mirror(features, target, proto, seen, inv_tau, pixel_weight=None, image_weight=None, batch=1, reduction="mean"):
    """``udaseg_proto_contrast_fwd_bwd``'s contract in numpy float64.  ``features [P, D]``; ``target``: an integer ``[P]`` array
    (hard labels) or a float ``[P, C]`` array (a distribution per pixel); ``proto [C, D]`` (rounded to float32 first), ``seen
    [C]``; ``pixel_weight [P]``, ``image_weight [batch]`` (``P = batch * pixels per image``; their product is taken in float32, the
    number the kernel tests).  Returns ``(loss, grad [P, D], stats int64 [4], why [P])``: ``why`` 0 = the pixel counts, 1 = void
    by its weight, 2 = by its label or target, 3 = by a non-finite feature; ``stats`` counts them.  Needs no GPU."""
    if reduction not in CONTRAST_REDUCTIONS:
        raise ValueError(f"reduction must be one of {CONTRAST_REDUCTIONS}, got {reduction!r}")
    f, pr, seen = _mirror_operands(features, proto, seen)
    P, C = f.shape[0], pr.shape[0]
    if not isinstance(batch, (int, np.integer)) or batch < 1 or P % batch:
        raise ValueError(f"batch must divide the {P} pixels, got {batch}")
    it = np.float64(inv_tau)
    w = np.ones(P, dtype=np.float32) if pixel_weight is None else np.asarray(pixel_weight, dtype=np.float32).reshape(-1).copy()
    if w.shape != (P,):
        raise ValueError(f"pixel_weight must have {P} elements, got {w.shape}")
    if image_weight is not None:
        wi = np.asarray(image_weight, dtype=np.float32)
        if wi.shape != (batch,):
            raise ValueError(f"image_weight must be [{batch}], got {wi.shape}")
        with np.errstate(all="ignore"):
            w = (w * np.repeat(wi, P // batch)).astype(np.float32)
    tg = np.asarray(target)
    hard = tg.ndim == 1
    if (hard and (tg.shape != (P,) or tg.dtype.kind not in "iu")) or (not hard and tg.shape != (P, C)):
        raise ValueError(f"target must be an integer [{P}] or a float [{P}, {C}] array, got {tg.dtype} {tg.shape}")
    with np.errstate(all="ignore"):
        w_ok = (w > 0) & np.isfinite(w)
        if hard:
            inr = (tg >= 0) & (tg < C)
            t = np.zeros((P, C))
            t[np.nonzero(inr)[0], tg[inr]] = 1.0
            t_ok = inr & seen[np.where(inr, tg, 0)]
        else:
            t32 = tg.astype(np.float32)
            t_ok = ((t32 >= 0) & (t32 <= 1)).all(axis=1)
            t = np.where(seen[None, :] & t_ok[:, None], t32.astype(np.float64), 0.0)    # the mass on unseen classes is dropped
            t_ok &= t.sum(axis=1) > 0
        why = np.where(~w_ok, 1, np.where(~t_ok, 2, np.where(~np.isfinite(f).all(axis=1), 3, 0)))
        stats = np.array([(why == k).sum() for k in range(4)], dtype=np.int64)
        div = {"mean": float(P), "sum": 1.0}.get(reduction)
        if div is None:
            div = float(w[w_ok].astype(np.float64).sum())
        grad = np.zeros_like(f)
        live = np.nonzero(why == 0)[0]
        if not (it > 0) or not seen.any() or not len(live):
            return (0.0 if div else float("nan")), grad, stats, why
        a, L, s = _assignment(f[live], pr, seen, it)
        tl, wl = t[live], w[live].astype(np.float64)
        T = tl.sum(axis=1)
        l = (tl * -a).sum(axis=1) + T * L
        loss = (wl * l).sum() / div if div else float("nan")
        grad[live] = (2.0 * it * wl / div)[:, None] * ((T[:, None] * s - tl) @ pr) if div else 0.0
    return float(loss), grad, stats, why


# ------------------------------------------------------------------------------------------------------------ device side
def _nhwc(who, what, x, channels):
    """[N,channels,H,W] device tensor -> (padded NHWC fp32 buffer, row stride, n, h, w): zero-copy for the views ``forward_parts``
    and ``rectify`` hand out, one layout kernel otherwise (bf16 is widened first)."""
    buf, ld, n, _, h, w = A.scores_nchw(who, x, channels, what, max_classes=channels)
    return buf, ld, n, h, w


class PrototypeBank(A.DeviceState):
    """One prototype per class in a ``dim``-channel feature space, with its state on the device (module docstring):
    ``sums [C, D]``, ``sq [C]`` float64 and ``counts [C + 2]`` int64 (the accumulators of the batch), ``prototypes [C, D]``,
    ``spread [C]`` float64, ``seen [C]`` int32, ``last_counts [C + 2]`` int64 (the counts the last update used: per class, labels
    beyond the classes, non-finite pixels) and ``inv_tau [1]`` fp32.  Allocated on first use.  ``accumulate`` and ``update``
    enqueue one kernel each and do not synchronise."""

    def __init__(self, num_classes, dim=DECODER_DIM, momentum=0.999, min_pixels=16, tau="auto", tau_scale=1.0, device=None):
        self.num_classes, self.dim = A.int_in("PrototypeBank", "num_classes", num_classes, 1, 32), _check_dim(dim)
        self.momentum, self.min_pixels = _check_momentum(momentum), _check_min_pixels(min_pixels)
        self.tau, self.tau_scale = _check_tau(tau, tau_scale)
        self.device = torch.device(device) if device is not None else None
        self.sums = None
        self.updates = 0

    def _allocate(self, device):
        C, D = self.num_classes, self.dim
        z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=device)
        self.sums, self.sq, self.counts = z(C, D), z(C), z(C + 2, dtype=torch.int64)
        self.prototypes, self.spread, self.seen = z(C, D), z(C), z(C, dtype=torch.int32)
        self.last_counts = z(C + 2, dtype=torch.int64)
        self.inv_tau = torch.full((1,), 0.0 if self.tau is None else 1.0 / self.tau, dtype=torch.float32, device=device)
        self._before = z(C, D)              # the prototypes before the last update (report's `moved`)
        self._seen_before = z(C, dtype=torch.int32)

    def reset(self):
        """Forget everything: accumulators, prototypes, seen flags; a fixed temperature stays."""
        if self.sums is not None:
            for t in (self.sums, self.sq, self.counts, self.prototypes, self.spread, self.seen, self.last_counts, self._before,
                      self._seen_before):
                t.zero_()
            if self.tau is None:
                self.inv_tau.zero_()
        self.updates = 0
        return self

    def accumulate(self, features, labels_u8):
        """Adds ``[N,D,H,W]`` features (fp32 or bf16, as ``forward_parts`` yields them) under uint8 ``[N,H,W]`` labels to the
        accumulators.  One kernel (plus one layout kernel for a tensor that is not the padded NHWC view)."""
        who = "PrototypeBank.accumulate"
        n, _, h, w = A.scores_shape(who, features, self.dim, "features", self.dim)
        if not torch.is_tensor(labels_u8) or labels_u8.dtype != torch.uint8 or tuple(labels_u8.shape) != (n, h, w):
            raise ValueError(f"{who}: labels must be a uint8 [{n},{h},{w}] tensor, got "
                             f"{getattr(labels_u8, 'dtype', None)} {tuple(getattr(labels_u8, 'shape', ()))}")
        dev = self._ensure(A.same_gpu(who, features=features, labels=labels_u8)).device
        buf, ldf = A.padded_nhwc(features.detach())
        A.on_device(dev, K.proto_accumulate, buf, ldf, self.dim, labels_u8.contiguous(), n * h * w, self.num_classes, self.sums,
                    self.sq, self.counts)
        return self

    def update(self, clear=True):
        """Prototypes, spreads, seen flags and (``tau="auto"``) the temperature from the accumulated pixels; the accumulators
        are zeroed by the same kernel unless ``clear`` is False."""
        self._ensure()
        self._before.copy_(self.prototypes)
        self._seen_before.copy_(self.seen)
        A.on_device(self.device, K.proto_update, self.sums, self.sq, self.counts, self.num_classes, self.dim, self.momentum,
                    self.min_pixels,
                    self.tau_scale if self.tau is None else 0.0, clear, self.prototypes, self.spread, self.seen,
                    self.last_counts, self.inv_tau)
        self.updates += 1
        return self

    def report(self):
        """Plain dict, ONE host read: per class ``seen``, ``spread`` and ``moved`` (the Euclidean distance its prototype moved in
        the last update; 0 for a class first seen by it), ``last_counts`` (per class), ``last_void`` / ``last_nonfinite`` (the other two
        counters of the last update) and ``tau`` (inf while ``inv_tau`` is 0)."""
        self._ensure()
        C = self.num_classes
        moved = (self.prototypes - self._before).square().sum(dim=1).sqrt() * (self._seen_before != 0)
        packed = torch.cat([self.seen.double(), self.last_counts.double(), self.spread, moved, self.inv_tau.double()]).cpu().numpy()
        seen, last = packed[:C], packed[C:2 * C + 2]
        inv_tau = float(packed[4 * C + 2])
        return {"seen": [bool(v) for v in seen], "last_counts": [int(v) for v in last[:C]], "last_void": int(last[C]),
                "last_nonfinite": int(last[C + 1]), "spread": packed[2 * C + 2:3 * C + 2].tolist(),
                "moved": packed[3 * C + 2:4 * C + 2].tolist(), "tau": 1.0 / inv_tau if inv_tau > 0.0 else float("inf")}

    _STATE = ("sums", "sq", "counts", "prototypes", "spread", "seen", "last_counts", "inv_tau")

    def state_dict(self):
        self._ensure()
        state = {k: getattr(self, k).detach().cpu().clone() for k in self._STATE}
        state.update(num_classes=self.num_classes, dim=self.dim, momentum=self.momentum, min_pixels=self.min_pixels,
                     tau="auto" if self.tau is None else self.tau, tau_scale=self.tau_scale, updates=self.updates)
        return state

    def load_state_dict(self, state):
        """Restores the device state bit for bit; the bank's shape must match, its other settings are taken from ``state``."""
        if int(state["num_classes"]) != self.num_classes or int(state["dim"]) != self.dim:
            raise ValueError(f"PrototypeBank.load_state_dict: the state is for {state['num_classes']} classes x {state['dim']} "
                             f"channels, the bank for {self.num_classes} x {self.dim}")
        momentum, min_pixels = _check_momentum(state["momentum"]), _check_min_pixels(state["min_pixels"])
        tau, tau_scale = _check_tau(state["tau"], state["tau_scale"])
        self._ensure()
        for k in self._STATE:
            dst = getattr(self, k)
            src = state[k]
            if src.dtype != dst.dtype or src.shape != dst.shape:
                raise ValueError(f"PrototypeBank.load_state_dict: {k} must be {dst.dtype} {tuple(dst.shape)}")
            dst.copy_(src)
        self._before.copy_(self.prototypes)
        self._seen_before.copy_(self.seen)
        self.momentum, self.min_pixels, self.tau, self.tau_scale = momentum, min_pixels, tau, tau_scale
        self.updates = int(state["updates"])
        return self


def rectify(features, outputs, bank, probs=False):
    """``[N,C,H,W]`` rectified probabilities (a strided view of a padded NHWC buffer, which ``ConfidenceHistogram.update`` and
    ``pseudo_labels`` read in place with ``probs=True``) of ``[N,D,H,W]`` features and ``[N,C,H,W]`` logits (or probabilities with
    ``probs``) under ``bank``'s prototypes.  One kernel, no host sync."""
    if not isinstance(bank, PrototypeBank):
        raise ValueError(f"rectify: bank must be a PrototypeBank, got {type(bank).__name__}")
    C = bank.num_classes
    n, _, h, w = A.scores_shape("rectify", features, bank.dim, "features", bank.dim)
    if A.scores_shape("rectify", outputs, C) != (n, C, h, w):
        raise ValueError(f"rectify: scores must be a [{n},{C},{h},{w}] tensor, got {tuple(outputs.shape)}")
    dev = bank._ensure(A.same_gpu("rectify", features=features, scores=outputs)).device
    fbuf, ldf = A.padded_nhwc(features.detach())
    sbuf, ldc = A.padded_nhwc(outputs.detach())
    out = torch.empty((n, h, w, ldc), dtype=torch.float32, device=dev)
    A.on_device(dev, K.proto_rectify, fbuf, ldf, bank.dim, sbuf, ldc, C, probs, bank.prototypes, bank.seen, bank.inv_tau, n * h * w,
                out)
    return out.permute(0, 3, 1, 2)[:, :C]


def assign(features, bank):
    """``[N,C,H,W]`` soft assignment of ``[N,D,H,W]`` features to ``bank``'s seen prototypes: the softmax of ``-d / tau`` over
    them, a distribution per pixel (``assign_mirror`` states it; a strided view of a padded NHWC buffer, which
    ``PrototypeContrastLoss`` and ``SoftCrossEntropyLoss(probs=True)`` read in place).  NaN rows mark pixels with a non-finite
    feature.  One kernel, no host sync, no gradient."""
    if not isinstance(bank, PrototypeBank):
        raise ValueError(f"assign: bank must be a PrototypeBank, got {type(bank).__name__}")
    C = bank.num_classes
    fbuf, ldf, n, h, w = _nhwc("assign", "features", features, bank.dim)
    bank._ensure(features.device)
    ldc = (C + 3) // 4 * 4
    out = torch.empty((n, h, w, ldc), dtype=torch.float32, device=features.device)
    A.on_device(features.device, K.proto_assign, fbuf, ldf, bank.dim, C, ldc, bank.prototypes, bank.seen, bank.inv_tau, n * h * w, out)
    return out.permute(0, 3, 1, 2)[:, :C]


class _PrototypeContrastFunction(torch.autograd.Function):
    """``losses._SoftCrossEntropyFunction``'s shape on the features: for 'weighted_mean' one launch over the weights alone makes
    D; then ONE pass makes the loss and, when the features need a gradient, the gradient already scaled; backward only scales it
    if it has to.  A second backward through a retained graph re-runs the entry point."""

    @staticmethod
    def forward(ctx, features, fbuf, ldf, labels, tbuf, ldt, wpx, wimg, bank, reduction, stats, want_grad):
        n, d, h, w = features.shape
        dev = features.device
        denom = None
        if reduction == "weighted_mean":
            denom = torch.empty(1, device=dev, dtype=torch.float64)
            K.pixel_weight_sum(wpx, wimg, n, h * w, torch.empty(3 * K.seg_partials(), device=dev, dtype=torch.float64), denom,
                               torch.empty(2, device=dev, dtype=torch.int64))
        ctx.meta = (n, d, h, w, ldf, ldt, bank, reduction)
        ctx.save_for_backward(fbuf, labels, tbuf, wpx, wimg, denom)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        # want_grad: whether a graph is being recorded at all (inside forward grad mode is always off, and under no_grad
        # needs_input_grad still names a leaf that requires one)
        ctx.dfeat = _PrototypeContrastFunction._run(ctx.meta, fbuf, labels, tbuf, wpx, wimg, denom, loss, stats,
                                                    want_grad and ctx.needs_input_grad[0])
        return loss

    @staticmethod
    def _run(meta, fbuf, labels, tbuf, wpx, wimg, denom, loss, stats, grad):
        n, d, h, w, ldf, ldt, bank, reduction = meta
        dev = fbuf.device
        dfeat = torch.empty((n, h, w, ldf), device=dev, dtype=torch.float32) if grad else None
        K.proto_contrast_fwd_bwd(fbuf, ldf, d, labels, tbuf, ldt, wpx, wimg, n, h * w, bank.num_classes, bank.prototypes, bank.seen,
                                 bank.inv_tau, reduction == "mean", denom, torch.empty(K.seg_partials(), device=dev, dtype=torch.float64),
                                 loss, dfeat, stats)
        return dfeat

    @staticmethod
    def backward(ctx, grad_out):
        n, d, h, w = ctx.meta[:4]
        g = grad_out.detach().to(torch.float32).contiguous()
        dfeat, ctx.dfeat = ctx.dfeat, None                 # consumed: scaled in place below
        if dfeat is None:
            fbuf, labels, tbuf, wpx, wimg, denom = ctx.saved_tensors
            dfeat = _PrototypeContrastFunction._run(ctx.meta, fbuf, labels, tbuf, wpx, wimg, denom,
                                                    torch.empty((), device=fbuf.device, dtype=torch.float32), None, True)
        K.scale_unless_one(dfeat, g)
        return (dfeat.permute(0, 3, 1, 2)[:, :d],) + (None,) * 11


class PrototypeContrastLoss(torch.nn.Module):
    """Cross entropy between a pixel's soft assignment to ``bank``'s prototypes and a target over the classes, as a loss on the
    FEATURES: it pulls a feature toward the prototypes its target names and away from the others (module docstring,
    ``contrast_mirror`` states the arithmetic).  The prototypes receive no gradient: they are EMA state.

    ``forward(features [N,D,H,W], target, pixel_weight=None [N,H,W], image_weight=None [N]) -> scalar``.  ``features``: fp32 or
    bf16, as ``forward_parts(x, ("logits", "decoder"))`` yields them (read in place).  ``target``: a uint8 ``[N,H,W]`` mask (other
    integer masks are clamped to 0..255) -- ProCA's pixel-to-prototype contrast on labelled pixels -- or a float ``[N,C,H,W]``
    distribution (``assign``'s and ``rectify``'s outputs are read in place) -- ProDA's consistency between two views' assignments.
    A pixel is *void* -- loss and gradient exactly 0 -- when its weight is 0, negative or not finite; when its label is beyond the
    classes or names an unseen class; when its target row holds a value that is not finite or outside ``[0, 1]`` or has no mass on
    a seen class; when one of its features is not finite.  While the bank has seen no class or has no temperature yet the loss
    is 0.  ``reduction`` as ``SoftCrossEntropyLoss``.  ``last_stats``: device int64 ``[counted, void by weight, void by label or
    target, void by a non-finite feature]`` of the last call: read it when convenient."""

    REDUCTIONS = CONTRAST_REDUCTIONS

    def __init__(self, bank, reduction="mean"):
        super().__init__()
        if not isinstance(bank, PrototypeBank):
            raise ValueError(f"PrototypeContrastLoss: bank must be a PrototypeBank, got {type(bank).__name__}")
        if reduction not in self.REDUCTIONS:
            raise ValueError(f"PrototypeContrastLoss: reduction must be one of {self.REDUCTIONS}, got {reduction!r}")
        self.bank, self.reduction = bank, reduction
        self.last_stats = None

    def extra_repr(self):
        return f"classes={self.bank.num_classes}, dim={self.bank.dim}, reduction={self.reduction!r}"

    def forward(self, features, target, pixel_weight=None, image_weight=None):
        who = "PrototypeContrastLoss"
        C = self.bank.num_classes
        fbuf, ldf, n, h, w = _nhwc(who, "features", features, self.bank.dim)
        dev = features.device
        if not torch.is_tensor(target):
            raise ValueError(f"{who}: target must be a [{n},{h},{w}] integer mask or a [{n},{C},{h},{w}] float distribution, got "
                             f"{type(target).__name__}")
        if target.requires_grad:
            raise ValueError(f"{who}: the target never receives a gradient; pass target.detach()")
        for name, t, shape in (("pixel_weight", pixel_weight, (n, h, w)), ("image_weight", image_weight, (n,))):
            if t is None:
                continue
            if not torch.is_tensor(t) or tuple(t.shape) != shape or not t.is_floating_point():
                raise ValueError(f"{who}: {name} must be a floating-point tensor of shape {shape}, got "
                                 f"{tuple(getattr(t, 'shape', ()))}")
            if t.requires_grad:
                raise ValueError(f"{who}: {name} never receives a gradient; pass {name}.detach()")
        A.same_gpu(who, features=features, target=target, pixel_weight=pixel_weight, image_weight=image_weight)
        labels = tbuf = None
        ldt = 0
        if target.is_floating_point():
            if tuple(target.shape) != (n, C, h, w):
                raise ValueError(f"{who}: a soft target must be a [{n},{C},{h},{w}] tensor, got {tuple(target.shape)}")
            tbuf, ldt, _, _, _ = _nhwc(who, "target", target, C)
        else:
            if tuple(target.shape) != (n, h, w) or target.dtype == torch.bool:
                raise ValueError(f"{who}: a hard target must be a [{n},{h},{w}] integer mask, got {target.dtype} {tuple(target.shape)}")
            labels = (target if target.dtype == torch.uint8 else target.clamp(0, 255).to(torch.uint8)).contiguous()
        self.bank._ensure(dev)
        wpx = None if pixel_weight is None else pixel_weight.to(torch.float32).contiguous()
        wimg = None if image_weight is None else image_weight.to(torch.float32).contiguous()
        stats = torch.zeros(4, device=dev, dtype=torch.int64)
        out = A.on_device(dev, _PrototypeContrastFunction.apply, features, fbuf, ldf, labels, tbuf, ldt, wpx, wimg, self.bank,
                          self.reduction, stats, torch.is_grad_enabled())     # the backward runs on the device's autograd thread
        self.last_stats = stats
        return out


def domain_gap(bank_a, bank_b):
    """Per-class Euclidean distance between two banks' prototypes (a source bank against a target bank), NaN where either side
    has not seen the class: a ``[C]`` list, one host read."""
    for b in (bank_a, bank_b):
        if not isinstance(b, PrototypeBank):
            raise ValueError(f"domain_gap: two PrototypeBanks are needed, got {type(b).__name__}")
    if (bank_a.num_classes, bank_a.dim) != (bank_b.num_classes, bank_b.dim):
        raise ValueError(f"domain_gap: the banks differ in shape: {bank_a.num_classes} x {bank_a.dim} against "
                         f"{bank_b.num_classes} x {bank_b.dim}")
    bank_a._ensure()
    bank_b._ensure(bank_a.device)
    dist = (bank_a.prototypes - bank_b.prototypes).square().sum(dim=1).sqrt()
    both = (bank_a.seen != 0) & (bank_b.seen != 0)
    return torch.where(both, dist, torch.full_like(dist, float("nan"))).cpu().tolist()


class PrototypeLabeler(teacher.OnlineLabeler):
    """``OnlineLabeler`` whose probabilities pass through the prototypes (module docstring).  Every ``label`` call makes ONE
    eval-mode, no-grad ``forward_parts(images, ("logits", "decoder"))`` of the teacher; the raw winner of every finite pixel
    (``pseudo_labels`` under zero thresholds) feeds ``bank.accumulate`` and ``bank.update`` (unless ``update_bank`` is False), and
    from call number ``rectify_after`` on (calls count from 0) ``rectify``'s probabilities feed the confidence table, the
    thresholds and the labels; before that the raw logits do, exactly as in ``OnlineLabeler``.  No host read.
    ``bank``: a ``PrototypeBank`` of ``num_classes`` classes (None: one over the decoder's 16 channels with its defaults)."""

    def __init__(self, teacher, num_classes, portion=0.2, floor=0.0, cap=0.9, bins=pseudo.BINS, void=255, halve_every=None,
                 dtype=None, bank=None, rectify_after=0, update_bank=True):
        super().__init__(teacher, num_classes, portion, floor, cap, bins, void, halve_every, dtype)
        if bank is None:
            bank = PrototypeBank(self.num_classes, DECODER_DIM)
        if not isinstance(bank, PrototypeBank) or bank.num_classes != self.num_classes:
            raise ValueError(f"bank must be a PrototypeBank of {self.num_classes} classes, got "
                             f"{getattr(bank, 'num_classes', type(bank).__name__)}")
        if not hasattr(self.model, "forward_parts"):
            raise ValueError("PrototypeLabeler: the model must offer forward_parts(images, (\"logits\", \"decoder\")), as Unet does")
        self.bank = bank
        self.rectify_after = A.int_in("PrototypeLabeler", "rectify_after", rectify_after, 0)
        self.update_bank = bool(update_bank)
        self._zero_thr = None

    def _forward_parts(self, frames_u8, want):
        from .data import prepare_batch
        self.device                                         # a model on the CPU: "no CPU path"
        dtype = self.dtype or getattr(self.model, "compute_dtype", torch.float32)
        images, _ = prepare_batch(frames_u8, None, None, dtype)
        with A.eval_mode(self.model), torch.no_grad():
            return self.model.forward_parts(images, want)

    def _raw_winners(self, out):
        if self._zero_thr is None or self._zero_thr.device != out.device:
            self._zero_thr = torch.zeros(self.num_classes, dtype=torch.int32, device=out.device)
        return pseudo.pseudo_labels(out, self._zero_thr, self.void, bins=self.bins)

    def label(self, frames_u8):
        """uint8 ``[N,H,W]`` masks (device) of uint8 ``[N,H,W,3]`` frames; updates the bank, the table and ``self.thr_bins``.
        No host read."""
        out, dec = self._forward_parts(frames_u8, ("logits", "decoder"))
        if self.update_bank:
            self.bank.accumulate(dec, self._raw_winners(out))
            self.bank.update()
        probs = self.calls >= self.rectify_after
        scores = rectify(dec, out, self.bank) if probs else out
        if self.halve_every and self.calls and self.calls % self.halve_every == 0:
            self.halve_(self.hist.table)
        self.calls += 1
        self.hist.update(scores, probs=probs)
        self.thr_bins = self.hist.thresholds(self.portion, self.floor, self.cap)
        return pseudo.pseudo_labels(scores, self.thr_bins, self.void, probs=probs, bins=self.bins)

    def init_from(self, loader_u8, labelled=True):
        """Accumulates the bank over a loader of ``(frames_u8, masks_u8)`` batches (``labelled``; the masks' values beyond the
        classes count as void) or of frames alone (the raw winners label them), then runs ONE ``update``: source-initialised
        prototypes.  Eval-mode forwards; the model's training flag is restored."""
        batches = 0
        for batch in loader_u8:
            dev = self.device
            if labelled:
                if torch.is_tensor(batch) or len(batch) < 2:
                    raise ValueError("PrototypeLabeler.init_from: labelled=True needs (frames, masks) batches")
                frames, masks = batch[0].to(dev, non_blocking=True), batch[1].to(dev, non_blocking=True)
                if masks.dtype != torch.uint8:
                    masks = masks.clamp(0, 255).to(torch.uint8)
                dec = self._forward_parts(frames, ("decoder",))
            else:
                frames = pseudo._frames_of(batch).to(dev, non_blocking=True)
                out, dec = self._forward_parts(frames, ("logits", "decoder"))
                masks = self._raw_winners(out)
            self.bank.accumulate(dec, masks)
            batches += 1
        if not batches:
            raise ValueError("PrototypeLabeler.init_from: the loader yielded no batches")
        self.bank.update()
        return self

    def report(self):
        """``OnlineLabeler.report()``'s keys and ``PrototypeBank.report()``'s in one dict (no name is shared); two host reads."""
        rep = super().report()
        rep.update(self.bank.report())
        return rep
