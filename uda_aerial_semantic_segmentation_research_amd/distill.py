"""``DistillTrainer`` -- self-training on the teacher's whole DISTRIBUTION instead of a thresholded argmax.

``pseudo``, ``teacher``, ``mix`` and ``proto`` make better teacher outputs for unlabelled target frames, and until here the only
route from them into the student was a uint8 mask into ``CrossEntropyLoss(ignore_index=255)``.  This trainer feeds the
distribution itself to ``losses.SoftCrossEntropyLoss`` (soft cross entropy, KL, or the symmetric cross entropy ProDA's later
stages train with), weighted per image by the share of confident pixels (``pseudo.confidence_share``; DACS's and DAFormer's
``q_i``).  An EXTENSION: the reference has no counterpart.

One iteration (``distill_step``):

    teacher:   eval mode, no grad, ONE forward of the target batch: logits, or with ``bank`` logits and decoder features, which
               ``proto.rectify`` turns into rectified probabilities (``probs=True``; its NaN rows become void pixels of the loss)
    weights:   image_weight = confidence_share(teacher output, tau)                      (device fp32 [N], no host read)
    student:   zero_grad; logits_s = model(source), logits_t = model(target or its strongly augmented view);
               total = criterion(logits_s, labels) + lambda_soft * soft(logits_t, teacher output, image_weight=image_weight);
               total.backward(); optimizer.step(); teacher.update() for a ``MeanTeacher``

The teacher never receives a gradient.  With ``lambda_soft == 0`` the target forward still runs (its BatchNorm statistics move as
they would otherwise) and ``soft_loss`` is reported, but it is left out of the backward.  Data-parallel training is not
implemented for this trainer.
"""
import torch

from . import proto, pseudo
from .adversarial_trainer import _drop_channel_axis, _wrap_around
from .losses import SoftCrossEntropyLoss
from .optim import FusedAdam
from .teacher import MeanTeacher
from .train import SegmentationTrainer


class DistillTrainer(SegmentationTrainer):
    def __init__(self, model, device, teacher, lambda_soft=1.0, loss=None, tau=0.968, bank=None, criterion=None):
        """teacher: a ``MeanTeacher`` of ``model`` (updated after every optimiser step) or a frozen ``nn.Module``; loss: a
        ``SoftCrossEntropyLoss`` (None: ``SoftCrossEntropyLoss()``); tau: the confidence a pixel needs to count towards its image's
        weight (DACS: 0.968); bank: a ``proto.PrototypeBank`` whose prototypes rectify the teacher's output (None: raw logits)."""
        super().__init__(model, device, criterion=criterion)
        if isinstance(teacher, MeanTeacher):
            self.teacher, self.teacher_model = teacher, teacher.model
        elif isinstance(teacher, torch.nn.Module):
            if teacher is model:
                raise ValueError("DistillTrainer: the teacher must not be the student itself; use a MeanTeacher or a frozen copy")
            self.teacher_model = teacher.to(device)
        else:
            raise ValueError(f"DistillTrainer: teacher must be a MeanTeacher or a torch.nn.Module, got {type(teacher).__name__}")
        if loss is None:
            loss = SoftCrossEntropyLoss()
        if not isinstance(loss, SoftCrossEntropyLoss):
            raise ValueError(f"DistillTrainer: loss must be a SoftCrossEntropyLoss, got {type(loss).__name__}")
        if bank is not None:
            if not isinstance(bank, proto.PrototypeBank) or bank.num_classes != self.num_classes:
                raise ValueError(f"DistillTrainer: bank must be a PrototypeBank of {self.num_classes} classes, got "
                                 f"{getattr(bank, 'num_classes', type(bank).__name__)}")
            if not hasattr(self.teacher_model, "forward_parts"):
                raise ValueError("DistillTrainer: with a bank the teacher must offer forward_parts(images, (\"logits\", \"decoder\")), "
                                 "as Unet does")
        tau = float(tau)
        if not 0.0 <= tau <= 1.0:
            raise ValueError(f"DistillTrainer: tau must lie in [0, 1], got {tau}")
        self.lambda_soft = float(lambda_soft)
        self.soft_loss = loss
        self.tau = tau
        self.bank = bank
        self.last_losses = {}
        self.last_share = None            # device fp32 [N]: the image weights of the last step
        self.last_target_logits = None    # the student's target logits of the last step (detached view; tests, logging)

    def teacher_output(self, target_images):
        """(scores [N,C,H,W], probs): the teacher's eval-mode, no-grad view of a target batch -- logits, or rectified probabilities
        with a bank.  The teacher's training flag is restored."""
        net = self.teacher_model
        was = net.training
        net.eval()
        try:
            with torch.no_grad():
                if self.bank is None:
                    return net(target_images), False
                logits, dec = net.forward_parts(target_images, ("logits", "decoder"))
                return proto.rectify(dec, logits, self.bank), True
        finally:
            net.train(was)

    def distill_step(self, source_images, source_masks, target_images, optimizer, target_student_images=None):
        """One iteration.  ``target_student_images``: what the student sees of the target batch (a strongly augmented view of the
        same geometry; None: ``target_images``).  Returns (seg_loss, soft_loss, total, share) as device tensors and leaves them
        in ``last_losses`` (``share`` as the batch mean) as 0-dim device tensors: no host sync here, ``float()`` reads one."""
        if self.grad_reducer is not None:
            raise NotImplementedError("DistillTrainer: data-parallel training (a gradient reducer) is not supported: the segmenter "
                                      "takes two forwards per backward and its bucket schedule assumes one")
        labels = _drop_channel_axis(source_masks)
        scores, probs = self.teacher_output(target_images)
        share = pseudo.confidence_share(scores, self.tau, probs=probs)

        optimizer.zero_grad()
        student_view = target_images if target_student_images is None else target_student_images
        logits_s, logits_t = self.model(source_images), self.model(student_view)
        seg_loss = self.criterion(logits_s, labels)
        if self.lambda_soft != 0.0:
            soft = self.soft_loss(logits_t, scores, probs=probs, image_weight=share)
            total = seg_loss + self.lambda_soft * soft
        else:
            with torch.no_grad():
                soft = self.soft_loss(logits_t.detach(), scores, probs=probs, image_weight=share)
            total = seg_loss
        total.backward()
        optimizer.step()
        if self.teacher is not None:
            self.teacher.update()
        self.last_share, self.last_target_logits = share, logits_t.detach()
        self.last_losses = {"seg_loss": seg_loss.detach(), "soft_loss": soft.detach(), "total": total.detach(), "share": share.mean()}
        return seg_loss, soft.detach(), total, share

    def train_epoch(self, source_dataloader, target_dataloader, optimizer, epoch):
        """One epoch over the source loader of ``(images, masks)`` batches; the target loader of image batches wraps around.
        Returns the mean total loss; ``last_losses`` holds the last iteration's ``seg_loss``, ``soft_loss``, ``total`` and ``share``
        (the mean image weight) as floats."""
        self.model.train()
        running, batches = 0.0, 0
        for (images, masks), target in zip(source_dataloader, _wrap_around(target_dataloader)):
            seg, soft, tot, share = self.distill_step(images.to(self.device), masks.to(self.device).long(), target.to(self.device),
                                                      optimizer)
            seg, soft, tot, sh = torch.stack([seg.detach(), soft, tot.detach(), share.mean()]).tolist()    # one transfer per iteration
            self.last_losses = {"seg_loss": seg, "soft_loss": soft, "total": tot, "share": sh}
            running += tot
            batches += 1
        return running / max(batches, 1)

    def train(self, source_dataloader, target_dataloader, valid_dataloader, epochs, learning_rate, patience=7):
        optimizer = FusedAdam(self.model.parameters(), lr=learning_rate)
        best, stale = float("inf"), 0
        for epoch in range(1, epochs + 1):
            self.current_epoch = epoch
            train_loss = self.train_epoch(source_dataloader, target_dataloader, optimizer, epoch)
            valid = self.validate(valid_dataloader)
            print(f"Train Loss: {train_loss:.4f}")
            print(f"Valid Metrics: {valid}")
            stale = 0 if valid["loss"] < best else stale + 1
            best = min(best, valid["loss"])
            if stale >= patience:
                print(f"Early stopping after {epoch} epochs")
                break
