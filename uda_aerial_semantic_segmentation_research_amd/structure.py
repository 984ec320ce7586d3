"""``StructureTrainer`` -- ``DistillTrainer`` plus losses on the decoder FEATURES: target structure learning.

``proto.rectify`` and ``DistillTrainer`` only ever read the prototypes: every loss ends at the logits.  ProDA (Zhang et al. 2021),
ProCA (Jiang et al., ECCV 2022) and SePiCo (Xie et al. 2023) get their second gain from letting the prototypes shape the features.
This trainer adds the two terms to the distillation step, both through ``proto.PrototypeContrastLoss`` (one fused HIP pass each):

    source:  contrast(dec_s, source masks)                 a labelled pixel's feature is pulled toward its class prototype and away
                                                           from the others (ProCA's pixel-to-prototype contrast)
    target:  contrast(dec_t, assign(dec_teacher, bank),    the strong view's prototype assignment follows the teacher's assignment of
                      image_weight=share)                  the weak view (ProDA's structure consistency), weighted per image like the
                                                           soft loss

One iteration (``distill_step``):

    teacher:   eval mode, no grad, ONE forward of the target batch: logits and decoder features -> rectified probabilities
               (``proto.rectify``) for the soft loss, the prototype assignment (``proto.assign``) for the target term
    student:   ``forward_parts(x, ("logits", "decoder"))`` on the source batch and on the target (strong) view;
               total = seg + lambda_soft * soft + lambda_src * contrast_src + lambda_tgt * contrast_tgt;
               total.backward() -- the feature gradients enter the last decoder block beside the head's; optimizer.step();
               teacher.update() for a ``MeanTeacher``

A term whose lambda is 0 is computed under ``no_grad`` for the report and left out of the backward.  The prototypes receive no
gradient and this trainer does not move them: the bank is filled and updated by its owner (``proto.PrototypeLabeler``, or
``bank.accumulate`` / ``bank.update`` on the teacher's features between steps).  No host read in the step.  Data-parallel training
is not implemented for this trainer.  An EXTENSION: the reference has no counterpart.  Deviations from the papers: squared Euclidean
distance in the decoder's 16 channels, not cosine similarity in a 256-channel projection; one prototype per class and no memory bank
of negatives; the mass a soft target puts on classes the bank has not seen is dropped.
"""
import math

import torch

from . import proto, pseudo
from .adversarial_trainer import _drop_channel_axis
from .distill import DistillTrainer

PARTS = ("logits", "decoder")


class StructureTrainer(DistillTrainer):
    def __init__(self, model, device, teacher, bank, lambda_src=0.0, lambda_tgt=0.0, contrast=None, **distill):
        """bank: the ``proto.PrototypeBank`` (required) both the rectification and the feature losses read; lambda_src / lambda_tgt:
        the weights of the source and the target feature term; contrast: a ``proto.PrototypeContrastLoss`` on ``bank`` (None: one
        with its defaults); the other arguments are ``DistillTrainer``'s (``lambda_soft``, ``loss``, ``tau``, ``criterion``)."""
        if bank is None:
            raise ValueError("StructureTrainer: a PrototypeBank is required (the feature losses have nothing else to pull toward)")
        super().__init__(model, device, teacher, bank=bank, **distill)
        if not hasattr(self.model, "forward_parts"):
            raise ValueError("StructureTrainer: the model must offer forward_parts(images, (\"logits\", \"decoder\")), as Unet does")
        for name, v in (("lambda_src", lambda_src), ("lambda_tgt", lambda_tgt)):
            if not math.isfinite(float(v)):
                raise ValueError(f"StructureTrainer: {name} must be finite, got {v}")
        if contrast is None:
            contrast = proto.PrototypeContrastLoss(bank)
        if not isinstance(contrast, proto.PrototypeContrastLoss) or contrast.bank is not bank:
            raise ValueError("StructureTrainer: contrast must be a PrototypeContrastLoss on the trainer's bank")
        self.lambda_src, self.lambda_tgt = float(lambda_src), float(lambda_tgt)
        self.contrast = contrast
        self.last_assignment = None       # the teacher's prototype assignment of the last step ([N,C,H,W] view; tests, logging)

    def teacher_parts(self, target_images):
        """(rectified probabilities [N,C,H,W], prototype assignment [N,C,H,W]) from ONE eval-mode, no-grad forward of the teacher.
        The teacher's training flag is restored."""
        net = self.teacher_model
        was = net.training
        net.eval()
        try:
            with torch.no_grad():
                logits, dec = net.forward_parts(target_images, PARTS)
                return proto.rectify(dec, logits, self.bank), proto.assign(dec, self.bank)
        finally:
            net.train(was)

    def _term(self, weight, features, target, **kw):
        if weight != 0.0:
            return self.contrast(features, target, **kw)
        with torch.no_grad():
            return self.contrast(features.detach(), target, **kw)

    def distill_step(self, source_images, source_masks, target_images, optimizer, target_student_images=None):
        """One iteration (module docstring).  Returns (seg_loss, soft_loss, total, share) as ``DistillTrainer.distill_step`` and
        leaves them with ``src_contrast`` and ``tgt_contrast`` in ``last_losses`` as 0-dim device tensors: no host sync here."""
        if self.grad_reducer is not None:                      # the parent refuses, with its message, before touching anything
            return super().distill_step(source_images, source_masks, target_images, optimizer, target_student_images)
        labels = _drop_channel_axis(source_masks)
        scores, assignment = self.teacher_parts(target_images)
        share = pseudo.confidence_share(scores, self.tau, probs=True)

        optimizer.zero_grad()
        student_view = target_images if target_student_images is None else target_student_images
        logits_s, dec_s = self.model.forward_parts(source_images, PARTS)
        logits_t, dec_t = self.model.forward_parts(student_view, PARTS)
        seg_loss = self.criterion(logits_s, labels)
        total = seg_loss
        if self.lambda_soft != 0.0:
            soft = self.soft_loss(logits_t, scores, probs=True, image_weight=share)
            total = total + self.lambda_soft * soft
        else:
            with torch.no_grad():
                soft = self.soft_loss(logits_t.detach(), scores, probs=True, image_weight=share)
        src = self._term(self.lambda_src, dec_s, labels)
        tgt = self._term(self.lambda_tgt, dec_t, assignment, image_weight=share)
        if self.lambda_src != 0.0:
            total = total + self.lambda_src * src
        if self.lambda_tgt != 0.0:
            total = total + self.lambda_tgt * tgt
        total.backward()
        optimizer.step()
        if self.teacher is not None:
            self.teacher.update()
        self.last_share, self.last_target_logits, self.last_assignment = share, logits_t.detach(), assignment
        self.last_losses = {"seg_loss": seg_loss.detach(), "soft_loss": soft.detach(), "src_contrast": src.detach(),
                            "tgt_contrast": tgt.detach(), "total": total.detach(), "share": share.mean()}
        return seg_loss, soft.detach(), total, share

    def train_epoch(self, source_dataloader, target_dataloader, optimizer, epoch):
        """``DistillTrainer.train_epoch`` with the two feature terms in ``last_losses`` (floats; one transfer per iteration)."""
        from .adversarial_trainer import _wrap_around
        self.model.train()
        running, batches = 0.0, 0
        for (images, masks), target in zip(source_dataloader, _wrap_around(target_dataloader)):
            self.distill_step(images.to(self.device), masks.to(self.device).long(), target.to(self.device), optimizer)
            keys = list(self.last_losses)
            self.last_losses = dict(zip(keys, torch.stack([self.last_losses[k].float() for k in keys]).tolist()))
            running += self.last_losses["total"]
            batches += 1
        return running / max(batches, 1)
