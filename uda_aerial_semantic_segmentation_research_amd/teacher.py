"""Mean teacher for self-training on target frames: a network whose weights are the exponential moving average (EMA) of the
student's, updated on the device after every optimiser step, and a labeler that keeps its thresholds current from the teacher's
own batches.  An EXTENSION: the reference has no counterpart.  The method is Tarvainen & Valpola 2017; DACS, whose
mixing ``mix.py`` ships, takes its pseudo-labels from such a teacher, so that self-training does not chase its own noise.

The update (part of the public contract; ``udaseg_ema_flat``, include/udaseg.h, INTEGRATION.md "Mean teacher")
    ``decay_t = min(alpha, 1 - 1/(t+1))`` with ``t`` the number of updates already made (``warmup``; the first update is a copy,
    the second the mean of two students, ...) or ``alpha`` throughout.  ``w = float32(1 - decay_t)``; per element
    ``t <- fmaf(w, s - t, t)`` in fp32.  A network's parameters live in one flat fp32 arena (``engine.ArenaModule``), so one update
    is ONE launch over the two arenas, 12 bytes per parameter; the squared teacher-student distance comes out of the same pass.
    ``update()`` always asks for the distance, and that variant of the kernel is the slower one (its grid is capped at the 256
    partials of the reduction: 36 against 26 microseconds on the r18 arena, profiles/teacher_bench.txt).
    Eval-mode forwards re-fold BatchNorm into the weights on every call, so the teacher's next forward sees the update with no
    cache to invalidate.

BatchNorm running statistics (``buffers``): ``"copy"`` -- the teacher's are the student's (default); ``"ema"`` -- averaged like
the parameters; ``"keep"`` -- left alone.  The ``num_batches_tracked`` counters are copied under ``"copy"`` and ``"ema"``.

Data parallelism: every rank updates its own teacher from its own student.  The students are identical after every step (their
gradients are all-reduced), the update is deterministic, so the teachers stay identical: there is no communication.

Use::

    mt = teacher.MeanTeacher(model, alpha=0.99)
    labeler = teacher.OnlineLabeler(mt, num_classes=23, portion=0.2, cap=0.9, halve_every=100)
    mixed = mix.MixedLoader(source_loader_u8, labeler.loader(target_loader_u8), num_classes=23, generator=g)
    trainer = SegmentationTrainer(model, device, criterion=CrossEntropyLoss(ignore_index=255)); trainer.teacher = mt
    trainer.train_epoch(data.DeviceAugmentedLoader(mixed, generator=g), optimizer, epoch)
"""
import copy
import warnings

import torch

from . import pseudo
from .engine import ArenaModule

BUFFER_MODES = ("copy", "ema", "keep")


def _check_alpha(alpha):
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must lie in [0, 1], got {alpha}")
    return alpha


def ema_decay(t, alpha=0.99, warmup=True):
    """The decay of update number ``t`` (``t`` updates already made): ``min(alpha, 1 - 1/(t+1))`` with ``warmup``, else ``alpha``."""
    alpha = _check_alpha(alpha)
    if t < 0:
        raise ValueError(f"t must not be negative, got {t}")
    return min(alpha, 1.0 - 1.0 / (t + 1)) if warmup else alpha


def _layout(net):
    """What two arenas must share for one launch to cover them: length, per-entry offsets and physical shapes."""
    return (net._arena.numel(), net._buf_arena.numel(), net._nbt.numel(), [(o, n, shp) for _, o, n, shp, _, _ in net._entries])


class MeanTeacher:
    """EMA copy of ``student`` (module docstring).  ``.model``: a network of the student's class with its own storage, on the
    student's device, in eval mode, no parameter requiring a gradient; after construction its ``state_dict`` equals the student's
    bit for bit.  ``update()`` after every optimiser step (``SegmentationTrainer.teacher`` does it)."""

    def __init__(self, student, alpha=0.99, warmup=True, buffers="copy"):
        self.alpha = _check_alpha(alpha)
        self.warmup = bool(warmup)
        if buffers not in BUFFER_MODES:
            raise ValueError(f"buffers must be one of {BUFFER_MODES}, got {buffers!r}")
        self.buffers = buffers
        self._require_gpu(student)
        self.student = student
        if isinstance(student, ArenaModule):
            student.ensure_arena()
            self.model = student.clone_network()     # its own arenas, registered with engine.arena_owner
        else:
            self.model = copy.deepcopy(student)
        for p in self.model.parameters():
            p.requires_grad_(False)
        self.model.eval()
        self.step = 0
        self.flat_launches = 0                       # arena-wide kernel launches of the last update() (tests)
        self._dist2 = None                           # 0-dim fp64 on the device: |student - teacher|^2 after the last update
        self._warned = False
        self._laid = None                            # (student._entries, model._entries) of two arenas known to share a layout

    @staticmethod
    def _require_gpu(model):
        p = next(iter(model.parameters()), None)
        if p is None or p.device.type != "cuda":
            raise RuntimeError("MeanTeacher: the model must live on the GPU (no CPU path in this build)")
        return p.device

    def decay_at(self, t):
        return ema_decay(t, self.alpha, self.warmup)

    # ------------------------------------------------------------------------------------------------------ update
    def _same_layout(self):
        """True when one launch can cover the two networks' arenas; re-lays the teacher after the student was re-laid
        (``set_compute_dtype``, ``.to()``), values preserved."""
        s, t = self.student, self.model
        if not (isinstance(s, ArenaModule) and type(s) is type(t)):
            return False
        s.ensure_arena()
        if self._laid is not None and self._laid[0] is s._entries and self._laid[1] is t._entries and t._arena is not None:
            return True                              # both arenas as they were when last compared (build_arena makes new lists)
        self._laid = None
        if t._arena is not None and t._arena.device == s._arena.device and _layout(s) == _layout(t):
            self._laid = (s._entries, t._entries)
            return True
        if t.compute_dtype != s.compute_dtype:
            t.set_compute_dtype(s.compute_dtype)
        if next(t.parameters()).device != s._arena.device:
            t.to(s._arena.device)
        t.ensure_arena()
        if _layout(s) != _layout(t):
            return False
        self._laid = (s._entries, t._entries)
        return True

    def _ema(self, decay, buffers):
        from . import kernels as K
        from .optim import _dense_f32, _sumsq_scratch
        dev = self._require_gpu(self.student)
        scratch = _sumsq_scratch(dev)
        if self._dist2 is None or self._dist2.device != dev:
            self._dist2 = torch.zeros((), device=dev, dtype=torch.float64)
        self.flat_launches = 0
        if self._same_layout():
            s, t = self.student, self.model
            K.ema_flat(t._arena, s._arena, t._arena.numel(), decay, scratch, self._dist2)
            self.flat_launches += 1
            if buffers == "ema":
                K.ema_flat(t._buf_arena, s._buf_arena, t._buf_arena.numel(), decay)
                self.flat_launches += 1
            elif buffers == "copy":
                t._buf_arena.copy_(s._buf_arena)
            if buffers != "keep":
                t._nbt.copy_(s._nbt)
            return
        if not self._warned:
            warnings.warn("MeanTeacher: the teacher's and the student's parameters are not two arenas of one layout: the update "
                          "takes the per-tensor path -- same arithmetic, one launch per tensor instead of one per network", stacklevel=3)
            self._warned = True
        params = {k for k, _ in self.model.named_parameters()}
        ssd = self.student.state_dict()
        first = True
        for k, tv in self.model.state_dict().items():
            sv = ssd[k].to(tv.device)
            is_param = k in params
            if not is_param and (buffers == "keep" or buffers == "copy" or not tv.is_floating_point()):
                if buffers != "keep":
                    tv.copy_(sv)
                continue
            if _dense_f32(tv) and _dense_f32(sv):
                K.ema_flat(tv, sv, tv.numel(), decay, scratch if is_param else None, self._dist2 if is_param else None, not first)
            else:
                if decay == 0.0:
                    tv.copy_(sv)
                elif decay != 1.0:
                    tv.lerp_(sv.to(tv.dtype), float(torch.tensor(1.0 - decay, dtype=torch.float32)))
                if is_param:
                    d2 = (sv.double() - tv.double()).square().sum()
                    if first:
                        self._dist2.copy_(d2)
                    else:
                        self._dist2.add_(d2)
            if is_param:
                first = False

    @torch.no_grad()
    def update(self):
        """One EMA step at ``decay_at(self.step)``, then ``self.step += 1``.  No host synchronisation."""
        self._ema(self.decay_at(self.step), self.buffers)
        self.step += 1

    @torch.no_grad()
    def sync(self):
        """Hard copy of the student (parameters, running statistics, counters); ``step`` is unchanged."""
        self._ema(0.0, "copy")

    def distance(self):
        """L2 distance between the student's and the teacher's parameters right after the last update: 0-dim device tensor."""
        if self._dist2 is None:
            raise RuntimeError("MeanTeacher.distance: call update() first")
        return self._dist2.sqrt()

    # ------------------------------------------------------------------------------------------------- checkpoints
    def state_dict(self):
        from .checkpoint import dense_state_dict
        return {"model": dense_state_dict(self.model), "step": self.step, "alpha": self.alpha, "warmup": self.warmup,
                "buffers": self.buffers}

    def load_state_dict(self, state):
        """A resumed teacher continues its decay schedule."""
        if state["buffers"] not in BUFFER_MODES:
            raise ValueError(f"buffers must be one of {BUFFER_MODES}, got {state['buffers']!r}")
        alpha = _check_alpha(state["alpha"])
        self.model.load_state_dict(state["model"])
        self.step, self.alpha, self.warmup, self.buffers = int(state["step"]), alpha, bool(state["warmup"]), state["buffers"]


class OnlineLabeler(pseudo.PseudoLabeler):
    """``PseudoLabeler`` without the ``fit`` pass: every ``label`` call makes ONE eval-mode, no-grad forward of the teacher (a
    ``MeanTeacher`` or any model) and uses it three times -- it is added to the confidence table, the per-class thresholds are
    taken from the table as it then stands, and the frames are labelled under them; all on the device, with ``pseudo.py``'s
    kernels and contract.  ``halve_every``: every that many calls, before the table is updated, it is halved (an integer shift),
    so that the confidences of old teachers fade; None: never."""

    def __init__(self, teacher, num_classes, portion=0.2, floor=0.0, cap=0.9, bins=pseudo.BINS, void=255, halve_every=None,
                 dtype=None):
        if halve_every is not None and (not isinstance(halve_every, int) or halve_every < 1):
            raise ValueError(f"halve_every must be None or a positive integer, got {halve_every}")
        self.teacher = teacher if isinstance(teacher, MeanTeacher) else None
        super().__init__(teacher.model if self.teacher is not None else teacher, num_classes, portion, floor, cap, bins, void, dtype)
        self.halve_every = halve_every
        self.calls = 0

    @staticmethod
    def halve_(table):
        """In place ``table >>= 1`` on an int64 table."""
        return table.bitwise_right_shift_(1)

    def label(self, frames_u8):
        """uint8 ``[N,H,W]`` masks (device) of uint8 ``[N,H,W,3]`` frames; updates the table and ``self.thr_bins``.  No host read."""
        out = self._eval_forward(frames_u8)
        if self.halve_every and self.calls and self.calls % self.halve_every == 0:
            self.halve_(self.hist.table)
        self.calls += 1
        self.hist.update(out)
        self.thr_bins = self.hist.thresholds(self.portion, self.floor, self.cap)
        return pseudo.pseudo_labels(out, self.thr_bins, self.void, bins=self.bins)

    def loader(self, loader_u8):
        """Iterable (with ``__len__``) of ``(frames_u8, masks_u8)`` device batches, as ``PseudoLabeler.loader`` yields them."""
        return pseudo._LabelledLoader(self, loader_u8)

    def report(self):
        """``PseudoLabeler.report()``'s keys for the table as it stands; one host read."""
        if self.thr_bins is None:
            raise RuntimeError("OnlineLabeler.report: label a batch first")
        self._finish_fit()
        return dict(self._report)
