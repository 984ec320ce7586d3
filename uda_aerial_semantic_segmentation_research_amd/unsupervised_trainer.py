"""``UnsupervisedTrainer`` -- phase 3, unsupervised fine-tuning on the unlabelled target domain: the build's counterpart of
reference ``src/models/unsupervised_trainer.py:13-393``, with the whole iteration on the device.

Same constructor, ``train_epoch(target_dataloader, optimizer, epoch, supervised_dataloader=None) -> (mean loss, domain
metrics)``, ``validate``, ``train`` and ``early_stopping``.  One iteration (``finetune_step``), in the reference's order
(``:100-152``): two strongly augmented views of the target batch (``data.strong_views``: HIP kernels instead of two
albumentations calls per image on the host), two SEPARATE training-mode forwards of the model (BatchNorm sees each view's own
batch statistics and its running statistics move twice), the discriminator's verdict on the normalised un-augmented batch,
``FineTuningLoss``, a skip when the total is not finite (``:135-137``), then zero_grad, one backward through both live
plans, global-norm clipping at 1.0 over BOTH networks (``optim.clip_grad_norm_``, no host round trip) and the optimizer step.

Where this differs from the reference on purpose ("Phase 3"): the reference's third, discarded segmenter
forward on the un-augmented batch (``:122``) is not run; ``supervised=(images, masks)`` runs the segmenter on the images (the
reference passes the images themselves as ``supervised_pred``, ``:130``); ``autocast`` is the model's own ``compute_dtype``.
Kept as they are: the sigmoid applied to the discriminator's (already sigmoid) output for the metrics, with the same tensor as
source and target (``:149-152``).
"""
import math

import torch

from . import data
from .discriminator import DomainDiscriminator
from .domain_model import DomainAdaptationModel
from .losses import FineTuningLoss
from .metrics import DomainAdaptationMetrics
from .optim import FusedAdam, clip_grad_norm_
from .train import SegmentationTrainer

_LOGGED = ("total", "consistency", "domain_confusion", "supervised")


class UnsupervisedTrainer(SegmentationTrainer):
    def __init__(self, model, device, consistency_weight=1.0, domain_weight=0.1, supervised_weight=0.1, rampup_length=40,
                 log_interval=10, patience=7, augment=None, seed=0, clahe=False):
        """``augment``: callable for loaders that yield float ``[N,3,H,W]`` batches (called twice per batch, once per view);
        uint8 ``[N,H,W,3]`` batches take the device pipeline.  ``seed``: of the generator the augmentation records are drawn
        from.  ``clahe``: draw them with CLAHE switched on (``data.draw_strong_params``)."""
        if not isinstance(model, DomainAdaptationModel):
            dtype = getattr(model, "compute_dtype", torch.float32)
            model = DomainAdaptationModel(model, DomainDiscriminator(compute_dtype=dtype).to(device))
        super().__init__(model.to(device), device)
        self.fine_tuning_loss = FineTuningLoss(consistency_weight=consistency_weight, domain_weight=domain_weight,
                                               supervised_weight=supervised_weight, rampup_length=rampup_length)
        self.domain_metrics = DomainAdaptationMetrics()
        self.augment = augment
        self.clahe = clahe
        self.generator = torch.Generator().manual_seed(seed)
        self.log_interval = log_interval
        self.patience = patience
        self.max_grad_norm = 1.0
        self.best_score = float("-inf")
        self.best_epoch = 0
        self.counter = 0
        self.skipped = 0                 # iterations dropped because the total loss was not finite
        self.last_losses = {}
        self.last_grad_norm = None       # 0-dim device tensor of the last clipped step

    # Two backward passes accumulate into one gradient arena per step (ArenaModule.deliver_grads), which a GradAllReducer's
    # in-place bucket averaging cannot take: data-parallel phase 3 is not supported.
    @property
    def grad_reducer(self):
        return None

    @grad_reducer.setter
    def grad_reducer(self, value):
        if value is not None:
            raise RuntimeError("UnsupervisedTrainer: a GradAllReducer cannot be attached -- the two views' backward passes "
                               "accumulate into one gradient arena, which the reducer's in-place averaging does not support; "
                               "data-parallel phase 3 is out of scope")

    # ------------------------------------------------------------------------------------------------ one iteration
    def _views(self, target, params, clahe=None):
        dtype = getattr(self.model, "compute_dtype", torch.float32)
        if target.dtype == torch.uint8:
            n, h, w, _ = target.shape
            if params is None:
                clahe = self.clahe if clahe is None else clahe
                params = (data.draw_strong_params(n, h, w, self.generator, clahe),
                          data.draw_strong_params(n, h, w, self.generator, clahe))
            frames = target.to(self.device, non_blocking=True)
            view1, view2 = data.strong_views(frames, params[0], params[1], dtype=dtype)
            plain, _ = data.prepare_batch(frames, dtype=dtype)
            return view1, view2, plain
        if self.augment is None:
            raise ValueError("UnsupervisedTrainer: float batches need an `augment=` callable; uint8 [N,H,W,3] frames take the "
                             "device pipeline")
        plain = target.to(self.device)
        return self.augment(plain), self.augment(plain), plain

    def finetune_step(self, target_u8, optimizer, epoch, params=None, supervised=None, update_metrics=True, _events=None,
                      clahe=None):
        """The hot path.  ``target_u8``: uint8 ``[N,H,W,3]`` frames (or a float batch with ``augment=``); ``params``: a pair of
        ``data.StrongAugParams`` (drawn from the trainer's generator when None, with ``clahe`` -- the trainer's own setting when
        None -- passed to the draw); ``supervised``: ``(images, masks)`` or None.
        Returns the loss dict as device tensors, plus ``"skipped"`` (bool).  One host read: the finiteness check of the total,
        which fetches the logged scalars in the same transfer (``self.last_losses``).  ``_events``: a list that receives
        ``(phase, torch.cuda.Event)`` marks (tools/bench_finetune.py)."""
        def mark(phase):
            if _events is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                _events.append((phase, e))

        model = self.model
        mark("augment")
        view1, view2, plain = self._views(target_u8, params, clahe)
        mark("forward")
        pred1 = model(view1)
        pred2 = model(view2)
        domain_pred = model.discriminator(plain)
        sup_pred = sup_target = None
        if supervised is not None:
            images, masks = supervised
            if images.dtype == torch.uint8:
                images, _ = data.prepare_batch(images, dtype=getattr(model, "compute_dtype", torch.float32))
            sup_pred = model(images.to(self.device))
            sup_target = masks.to(self.device).long()
        mark("loss")
        loss_dict = self.fine_tuning_loss(pred1=pred1, pred2=pred2, domain_pred=domain_pred, epoch=epoch,
                                          supervised_pred=sup_pred, supervised_target=sup_target)
        values = torch.stack([loss_dict[k].detach().float() for k in _LOGGED]).tolist()
        self.last_losses = dict(zip(_LOGGED, values))
        self.last_losses["rampup_weight"] = float(loss_dict["rampup_weight"])
        loss_dict["skipped"] = not math.isfinite(values[0])
        if loss_dict["skipped"]:
            self.skipped += 1
            print(f"Warning: Invalid loss value encountered: {self.last_losses}")
            mark("end")
            return loss_dict
        mark("backward")
        optimizer.zero_grad()
        loss_dict["total"].backward()
        mark("clip")
        self.last_grad_norm = clip_grad_norm_(model.parameters(), self.max_grad_norm)
        mark("adam")
        optimizer.step()
        if self.teacher is not None:
            self.teacher.update()
        mark("end")
        if update_metrics:
            verdict = torch.sigmoid(domain_pred.detach())
            self.domain_metrics.update(source_pred=verdict, target_pred=verdict)
        return loss_dict

    # ------------------------------------------------------------------------------------------------------ epochs
    def train_epoch(self, target_dataloader, optimizer, epoch, supervised_dataloader=None, params=None):
        """``params``: a fixed pair of augmentation records for every iteration (tests, ablations); None draws fresh ones."""
        self.model.train()
        self.domain_metrics.reset()
        total_loss, num_batches = 0.0, 0
        supervised_iter = iter(supervised_dataloader) if supervised_dataloader else None
        for batch_idx, target in enumerate(target_dataloader):
            if isinstance(target, (list, tuple)):
                target = target[0]
            supervised = None
            if supervised_iter is not None:
                try:
                    supervised = next(supervised_iter)
                except StopIteration:
                    supervised_iter = iter(supervised_dataloader)
                    supervised = next(supervised_iter)
            out = self.finetune_step(target, optimizer, epoch, params=params, supervised=supervised)
            if out["skipped"]:
                continue
            total_loss += self.last_losses["total"]
            num_batches += 1
            if batch_idx % self.log_interval == 0:
                step = epoch * len(target_dataloader) + batch_idx if hasattr(target_dataloader, "__len__") else batch_idx
                for k, v in self.last_losses.items():
                    self.logger.log_scalar(f"train/loss_{k}", v, step)
                for k, v in self.domain_metrics.get_metrics().items():
                    self.logger.log_scalar(f"train/{k}", float(v), step)
                if self.teacher is not None:
                    self._log_teacher(step)
        return total_loss / max(num_batches, 1), self.domain_metrics.get_metrics()

    def validate(self, dataloader):
        """Mean IoU / accuracy of the segmenter over a labelled loader (reference ``:274-312``) -> metrics dict with ``'iou'``."""
        self.model.eval()
        self.valid_dataloader = dataloader
        iou = acc = 0.0
        n = 0
        metrics = {}
        with torch.no_grad():
            for images, masks in dataloader:
                if images.dtype == torch.uint8:
                    images, _ = data.prepare_batch(images, dtype=getattr(self.model, "compute_dtype", torch.float32))
                outputs = self.model(images.to(self.device))
                metrics = self.calculate_metrics(outputs, masks.to(self.device).long())
                iou += float(metrics.get("iou", 0))
                acc += float(metrics.get("accuracy", 0))
                n += 1
        metrics = dict(metrics)
        metrics["iou"] = iou / max(n, 1)
        metrics["accuracy"] = acc / max(n, 1)
        for k in ("iou", "accuracy"):
            self.logger.log_scalar(f"val/{k}", metrics[k], self.current_epoch)
        return metrics

    def train(self, target_dataloader, valid_dataloader, epochs, learning_rate, supervised_dataloader=None, patience=7):
        self.patience = patience
        optimizer = FusedAdam(self.model.parameters(), lr=learning_rate)
        for epoch in range(1, epochs + 1):
            self.current_epoch = epoch
            train_loss, train_metrics = self.train_epoch(target_dataloader, optimizer, epoch, supervised_dataloader)
            valid_metrics = self.validate(valid_dataloader)
            print(f"\nEpoch {epoch}:")
            print(f"Train Loss: {train_loss:.4f}")
            print(f"Train Metrics: {train_metrics}")
            print(f"Valid Metrics: { {k: v for k, v in valid_metrics.items() if not k.startswith('iou_class_')} }")
            if self.early_stopping(epoch, valid_metrics):
                print("Early stopping triggered")
                break

    def early_stopping(self, epoch, metrics):
        """Patience on the validation IoU (reference ``:361-393``): True when it has not improved for ``patience`` epochs."""
        score = float(metrics.get("iou", 0))
        if score > self.best_score:
            self.best_score, self.best_epoch, self.counter = score, epoch, 0
        else:
            self.counter += 1
        self.logger.log_scalar("early_stopping/score", score, epoch)
        self.logger.log_scalar("early_stopping/counter", self.counter, epoch)
        if self.counter >= self.patience:
            print(f"\nEarly stopping triggered. Best score: {self.best_score:.4f} at epoch {self.best_epoch}")
            return True
        return False
