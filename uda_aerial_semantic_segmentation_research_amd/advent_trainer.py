"""``AdventTrainer`` -- adversarial adaptation in the output space (AdvEnt, Vu et al., CVPR 2019), on ``AdversarialTrainer``'s surface.

``AdversarialTrainer`` keeps the reference's behaviour: its discriminator judges raw images, so ``lambda_adv * BCE(D(target))``
adds nothing to the segmenter's gradients.  Here the discriminator judges the weighted self-information maps of the
segmenter's *prediction* (``advent.self_information``), so the domain loss trains the whole segmenter through its logits, and the
direct part ``lambda_ent * EntropyLoss(target prediction)`` can be added; neither needs a target label.

One iteration runs in AdvEnt's order, which differs from ``AdversarialTrainer``'s (discriminator first, three discriminator
forwards, images as its input): the segmenter step comes first and the discriminator step reuses its predictions, so no forward
is repeated.

    segmenter:      zero_grad; logits_s = model(source), logits_t = model(target); seg = criterion(logits_s, labels);
                    maps_t = self_information(logits_t); adv = lambda_adv * BCE(D(maps_t), 1);
                    ent = lambda_ent * EntropyLoss(logits_t) (skipped entirely at lambda_ent == 0);
                    (seg + adv + ent).backward(); optimizer.step(); teacher update
    discriminator:  zero_grad (which also clears what the segmenter step's backward left in D's .grad);
                    d_loss = (BCE(D(self_information(logits_s.detach())), 1) + BCE(D(maps_t.detach()), 0)) / 2; backward; step

The label convention (source 1, target 0), the ``AdversarialLoss`` object, ``train_epoch`` / ``validate`` / ``train`` and the lazy
discriminator optimiser are ``AdversarialTrainer``'s.  Data-parallel training is not implemented for this trainer.
"""
import torch

from .advent import OutputSpaceDiscriminator, self_information
from .adversarial_trainer import AdversarialTrainer, _drop_channel_axis
from .losses import EntropyLoss


class AdventTrainer(AdversarialTrainer):
    def __init__(self, model, device, lambda_adv=0.001, lambda_ent=0.0, entropy_kind="entropy", criterion=None):
        super().__init__(model, device, lambda_adv=lambda_adv, criterion=criterion)
        # the image-level discriminator the base class built is replaced before anything used it
        self.discriminator = OutputSpaceDiscriminator(self.num_classes, compute_dtype=getattr(model, "compute_dtype", torch.float32)).to(device)
        self.lambda_ent = float(lambda_ent)
        self.entropy_loss = EntropyLoss(entropy_kind)

    def advent_step(self, source_images, source_masks, target_images, optimizer, update_metrics=True):
        """One iteration.  Returns (seg_loss, d_loss, adv_loss, ent_loss, total) as device tensors."""
        if self.grad_reducer is not None or self.d_grad_reducer is not None:
            raise NotImplementedError("AdventTrainer: data-parallel training (a gradient reducer) is not supported: the segmenter "
                                      "takes two forwards per backward and its bucket schedule assumes one")
        D, L = self.discriminator, self.adversarial_loss
        labels = _drop_channel_axis(source_masks)
        dt = D.compute_dtype

        # (1) segmenter: supervised on source; on target, fool D through the prediction (+ minimise its entropy)
        optimizer.zero_grad()
        logits_s, logits_t = self.model(source_images), self.model(target_images)
        seg_loss = self.criterion(logits_s, labels)
        maps_t = self_information(logits_t, dt)
        adv_loss = L.generator_loss(D(maps_t))
        total = seg_loss + adv_loss
        if self.lambda_ent != 0.0:
            ent_loss = self.lambda_ent * self.entropy_loss(logits_t)
            total = total + ent_loss
        else:
            ent_loss = torch.zeros((), device=seg_loss.device)
        total.backward()
        optimizer.step()
        if self.teacher is not None:
            self.teacher.update()

        # (2) discriminator: source predictions should score 1, target predictions 0
        self.discriminator_optimizer.zero_grad()
        verdict_src = D(self_information(logits_s.detach(), dt))
        verdict_tgt = D(maps_t.detach())
        if update_metrics:
            self.domain_metrics.update(verdict_src, verdict_tgt)
        d_loss = L.discriminator_loss(verdict_src, verdict_tgt)
        d_loss.backward()
        self.discriminator_optimizer.step()
        return seg_loss, d_loss, adv_loss, ent_loss.detach(), total

    def adversarial_step(self, source_images, source_masks, target_images, optimizer, update_metrics=True):
        """``train_epoch``'s hook: the AdvEnt iteration; ``last_losses`` gains ``ent_loss``."""
        seg, dl, adv, ent, tot = self.advent_step(source_images, source_masks, target_images, optimizer, update_metrics)
        self._ent = ent
        return seg, dl, adv, tot

    def train_epoch(self, source_dataloader, target_dataloader, optimizer, epoch):
        out = super().train_epoch(source_dataloader, target_dataloader, optimizer, epoch)
        if self.last_losses:
            self.last_losses["ent_loss"] = float(self._ent)
        return out
