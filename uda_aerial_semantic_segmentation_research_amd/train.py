"""``SegmentationTrainer`` -- the build's counterpart of reference ``src/models/train.py::SegmentationTrainer``
(``:197-503``): same constructor, ``train_epoch`` / ``validate`` / ``train`` / ``calculate_metrics`` signatures and
return shapes, same step order (``:336-346``: zero_grad -> forward -> CrossEntropy -> backward -> Adam step), with the
model, loss and optimizer running on the HIP kernels.  ``EarlyStopping`` restates ``:79-195``.

The reference's confusion-matrix / ROC / PR logging (``:245-328``, called at ``:374-379`` and ``:413-417``) is opt-in here
(``trainer.log_curves = True``): instead of sorting ``softmax(outputs)`` on the host class by class with sklearn it reads ONE
pair of per-class score histograms made on the device (``curves.py``).  Left out on purpose (OUT OF SCOPE): the
torchmetrics objects; TensorBoard logging degrades to a no-op when the package is absent.
"""
import os
from pathlib import Path

import numpy as np
import torch

from .config import Config
from .losses import CrossEntropyLoss
from .metrics import segmentation_metrics
from .optim import FusedAdam


class NullLogger:
    """Stand-in for the reference's TensorboardLogger (src/visualization/tensorboard_logger.py:11-86)."""

    def __init__(self, log_dir=None):
        self.log_dir = log_dir
        self.scalars = {}

    def log_scalar(self, tag, value, step):
        self.scalars.setdefault(tag, []).append((step, float(value)))

    def log_scalars(self, main_tag, tag_scalar_dict, step):
        for k, v in tag_scalar_dict.items():
            self.log_scalar(f"{main_tag}/{k}", v, step)

    def log_image(self, *a, **k):
        pass

    log_images = log_figure = log_histogram = log_model_graph = log_image

    def close(self):
        pass


class EarlyStopping:
    """Weighted multi-metric early stopping (reference train.py:79-195), including its ``min_epochs`` gate."""

    def __init__(self, patience=7, min_delta=0.0, mode="min", min_epochs=10, metrics_to_track=None, weights=None,
                 verbose=False):
        self.patience, self.min_delta, self.mode, self.min_epochs = patience, min_delta, mode, min_epochs
        self.metrics_to_track = metrics_to_track or ["loss"]
        self.weights = weights or {"loss": 1.0}
        self.verbose = verbose
        self.counter = 0
        self.best_score = None
        self.early_stop = False
        self.best_metrics = {}
        self.val_loss_min = float("inf")
        self.metric_history = {m: [] for m in self.metrics_to_track}

    def _calculate_score(self, metrics):
        return sum(self.weights[m] * v for m, v in metrics.items() if m in self.weights)

    def _is_better(self, current, best):
        return current < best - self.min_delta if self.mode == "min" else current > best + self.min_delta

    def __call__(self, epoch, metrics, logger=None):
        for m, v in metrics.items():
            if m in self.metric_history:
                self.metric_history[m].append(v)
        score = self._calculate_score(metrics)
        if logger:
            logger.log_scalar("early_stopping/score", score, epoch)
            logger.log_scalar("early_stopping/counter", self.counter, epoch)
        if epoch < self.min_epochs:
            return False
        if self.best_score is None or self._is_better(score, self.best_score):
            first = self.best_score is None
            self.best_score, self.best_metrics = score, metrics.copy()
            if not first:
                self.counter = 0
        else:
            self.counter += 1
            if self.verbose:
                print(f"EarlyStopping counter: {self.counter} out of {self.patience}")
            if self.counter >= self.patience:
                self.early_stop = True
                return True
        return False

    def get_best_metrics(self):
        return self.best_metrics

    def get_improvement_rate(self):
        return {m: (h[-1] - h[0]) / len(h) for m, h in self.metric_history.items() if len(h) > 1}


class SegmentationTrainer:
    def __init__(self, model, device, criterion=None):
        """model: segmentation model; device: device to train on; criterion: the segmentation loss (None: ``CrossEntropyLoss()``,
        e.g. ``CrossEntropyLoss(weight=w, ignore_index=255)`` for masks with void labels)."""
        self.model = model.to(device)
        self.device = device
        self.criterion = CrossEntropyLoss() if criterion is None else (criterion.to(device) if isinstance(criterion, torch.nn.Module)
                                                                          else criterion)
        self.logger = NullLogger(log_dir=Config.LOGS_DIR)
        self.num_classes = getattr(model, "classes", Config.NUM_CLASSES)
        self.log_metrics = True           # the reference computes metrics every batch; switch off for pure throughput
        self.grad_reducer = None          # ddp.GradAllReducer when data-parallel
        self.current_epoch = 0
        self.log_curves = False           # per-class ROC / PR curves, AUC and AP every Config.LOG_INTERVAL batches (reference :374-379)
        self.last_curves = {}             # prefix ('train' / 'val') -> the curves.curves_from_hist dict of the last logging call
        self.log_predictions = False      # image / ground truth / prediction / overlay of the batch's first sample, same schedule (reference _log_predictions)
        self.last_renders = {}            # 'image' / 'ground_truth' / 'prediction' / 'overlay' -> uint8 [H,W,3] on the device, of the last logging call
        self.teacher = None               # teacher.MeanTeacher: updated right after every optimiser step of the segmenter

    def calculate_metrics(self, outputs, masks):
        """Per-batch IoU / accuracy / per-class IoU (same keys as the reference)."""
        return segmentation_metrics(outputs, masks, self.num_classes)

    def _log_curves(self, outputs, masks, step, prefix):
        """What reference :374-379 / :413-417 log, from one device->host read: scalars ``{prefix}/auc_class_{c}``,
        ``{prefix}/ap_class_{c}`` for the classes with a finite value, ``{prefix}/mean_auc``, ``{prefix}/mean_ap``; the curve arrays
        stay on ``self.last_curves[prefix]``.  A logger other than the NullLogger that has ``log_figure`` also gets the reference's
        figures ``{prefix}/roc_curves``, ``{prefix}/pr_curves``, ``{prefix}/confusion_matrix`` when matplotlib imports."""
        from .curves import ScoreHistogram, curves_from_hist
        from .metrics import confusion_matrix
        k = self.num_classes
        hist = ScoreHistogram(k, device=outputs.device).update(outputs, masks)
        figures = hasattr(self.logger, "log_figure") and not isinstance(self.logger, NullLogger)
        if figures:
            try:
                from matplotlib.figure import Figure
            except ImportError:
                figures = False
        parts = [hist.tables.reshape(-1)]
        if figures:
            parts.append(confusion_matrix(outputs, masks, k).reshape(-1))
        packed = torch.cat(parts).cpu().numpy()                         # the ONE host read of this logging call
        tab = packed[:2 * k * hist.bins].reshape(2, k, hist.bins)
        cur = curves_from_hist(tab[0], tab[1], hist.score_range)
        self.last_curves[prefix] = cur
        for name in ("auc", "ap"):
            vals = cur[name]
            finite = np.isfinite(vals)
            for c in np.nonzero(finite)[0]:
                self.logger.log_scalar(f"{prefix}/{name}_class_{c}", vals[c], step)
            if finite.any():
                self.logger.log_scalar(f"{prefix}/mean_{name}", float(vals[finite].mean()), step)
        if not figures:
            return
        for tag, xs, ys, val, xl, yl in (("roc_curves", "fpr", "tpr", "auc", "False Positive Rate", "True Positive Rate"),
                                         ("pr_curves", "recall", "precision", "ap", "Recall", "Precision")):
            fig = Figure(figsize=(10, 8))
            ax = fig.subplots()
            for c in range(k):
                if np.isfinite(cur[val][c]):
                    ax.plot(cur[xs][c], cur[ys][c], label=f"Class {c} ({val.upper()} = {cur[val][c]:.2f})")
            if tag == "roc_curves":
                ax.plot([0, 1], [0, 1], "k--")
            ax.set_xlabel(xl)
            ax.set_ylabel(yl)
            ax.set_title(f"{prefix.capitalize()} {'ROC' if tag == 'roc_curves' else 'Precision-Recall'} Curves")
            ax.legend(fontsize="small")
            self.logger.log_figure(f"{prefix}/{tag}", fig, step)
        cm = packed[2 * k * hist.bins:].reshape(k, k)
        fig = Figure(figsize=(10, 8))
        ax = fig.subplots()
        ax.imshow(cm, cmap="Blues")
        for i in range(k):
            for j in range(k):
                ax.text(j, i, str(int(cm[i, j])), ha="center", va="center", fontsize=6)
        ax.set_xlabel("Predicted")
        ax.set_ylabel("True")
        ax.set_title(f"{prefix.capitalize()} Confusion Matrix")
        self.logger.log_figure(f"{prefix}/confusion_matrix", fig, step)

    def _log_predictions(self, images, masks, outputs, step, prefix):
        """The reference's ``_log_predictions`` with pictures made on the device (render.py): the first sample of the batch as
        ``{prefix}/image`` (the model input de-normalised), ``/ground_truth`` and ``/prediction`` (colour masks, void labels in the
        void colour) and ``/overlay`` (the prediction's colours over the image at 0.5), each handed to ``logger.log_image`` as a uint8
        ``[3,H,W]`` device tensor; the ``[H,W,3]`` pictures stay on ``self.last_renders``."""
        from . import kernels as K, render
        from ._args import logits_nhwc
        k = self.num_classes
        logits = outputs[:1]
        _, c, h, w = logits.shape
        buf, ldc = logits_nhwc(logits)
        pred = torch.empty((1, h, w), dtype=torch.int64, device=buf.device)
        K.predict_finish(buf, None, h * w, c, ldc, pred)
        pics = {"image": render.overlay(images[:1], pred, alpha=0.0, classes=k),
                "ground_truth": render.colorize(masks[:1], classes=k),
                "prediction": render.colorize(pred, classes=k),
                "overlay": render.overlay(images[:1], pred, alpha=0.5, classes=k)}
        self.last_renders = {name: p[0] for name, p in pics.items()}
        for name, p in self.last_renders.items():
            self.logger.log_image(f"{prefix}/{name}", p.permute(2, 0, 1), step)

    def _log_teacher(self, step):
        """``train/teacher_decay`` (the decay of the last update) and ``train/teacher_distance`` (|student - teacher| after it)."""
        self.logger.log_scalar("train/teacher_decay", self.teacher.decay_at(self.teacher.step - 1), step)
        self.logger.log_scalar("train/teacher_distance", float(self.teacher.distance()), step)

    def train_step(self, images, masks, optimizer):
        """The timed hot path: reference train.py:340-344.  Returns (loss tensor, logits), no host sync."""
        optimizer.zero_grad()
        outputs = self.model(images)
        loss = self.criterion(outputs, masks)
        loss.backward()
        if self.grad_reducer is not None:
            self.grad_reducer.finish()
        optimizer.step()
        if self.teacher is not None:
            self.teacher.update()
        return loss, outputs

    def train_epoch(self, dataloader, optimizer, epoch):
        """Train for one epoch; returns the mean loss."""
        self.model.train()
        total_loss = 0.0
        for batch_idx, (images, masks) in enumerate(dataloader):
            images = images.to(self.device)
            masks = masks.to(self.device).long()
            loss, outputs = self.train_step(images, masks, optimizer)
            total_loss += loss.item()
            if self.log_metrics:
                with torch.no_grad():
                    metrics = self.calculate_metrics(outputs.detach(), masks)
                step = (epoch - 1) * len(dataloader) + batch_idx
                self.logger.log_scalar("train/loss", total_loss / (batch_idx + 1), step)
                self.logger.log_scalar("train/iou", metrics["iou"], step)
                self.logger.log_scalar("train/accuracy", metrics["accuracy"], step)
                self.logger.log_scalar("train/learning_rate", optimizer.param_groups[0]["lr"], step)
                if self.teacher is not None and batch_idx % Config.LOG_INTERVAL == 0:
                    self._log_teacher(step)
            if self.log_curves and batch_idx % Config.LOG_INTERVAL == 0:
                with torch.no_grad():
                    self._log_curves(outputs.detach(), masks, (epoch - 1) * len(dataloader) + batch_idx, "train")
            if self.log_predictions and batch_idx % Config.LOG_INTERVAL == 0:
                with torch.no_grad():
                    self._log_predictions(images, masks, outputs.detach(), (epoch - 1) * len(dataloader) + batch_idx, "train")
        return total_loss / len(dataloader)

    def validate(self, dataloader):
        """Validate the model; returns {'loss','iou','accuracy'}."""
        self.model.eval()
        total_loss = 0.0
        all_metrics = []
        with torch.no_grad():
            for batch_idx, (images, masks) in enumerate(dataloader):
                images = images.to(self.device)
                masks = masks.to(self.device).long()
                outputs = self.model(images)
                loss = self.criterion(outputs, masks)
                total_loss += loss.item()
                metrics = self.calculate_metrics(outputs, masks)
                all_metrics.append(metrics)
                if batch_idx % Config.LOG_INTERVAL == 0:
                    for c in range(self.num_classes):
                        self.logger.log_scalar(f"val/iou_class_{c}", metrics[f"iou_class_{c}"], self.current_epoch)
                    if self.log_curves:
                        self._log_curves(outputs, masks, self.current_epoch, "val")
                    if self.log_predictions:
                        self._log_predictions(images, masks, outputs, self.current_epoch, "val")
        avg = {"loss": total_loss / len(dataloader),
               "iou": float(np.mean([m["iou"] for m in all_metrics])),
               "accuracy": float(np.mean([m["accuracy"] for m in all_metrics]))}
        for k, v in avg.items():
            self.logger.log_scalar(f"val/{k}", v, self.current_epoch)
        return avg

    def train(self, train_dataloader, valid_dataloader, epochs, learning_rate, patience=7):
        """Train the model (Adam, early stopping on a weighted loss/IoU/accuracy score, best-checkpoint save)."""
        optimizer = FusedAdam(self.model.parameters(), lr=learning_rate)
        early_stopping = EarlyStopping(patience=patience, mode="max", min_epochs=10, metrics_to_track=["loss", "iou", "accuracy"],
                                       weights={"loss": -1.0, "iou": 1.0, "accuracy": 0.5}, verbose=True)
        self.current_epoch = 0
        for epoch in range(1, epochs + 1):
            self.current_epoch = epoch
            train_loss = self.train_epoch(train_dataloader, optimizer, epoch)
            valid_metrics = self.validate(valid_dataloader)
            print(f"Train Loss: {train_loss:.4f}")
            print(f"Valid Loss: {valid_metrics['loss']:.4f}")
            print(f"Valid Metrics: {valid_metrics}")
            if early_stopping(epoch, valid_metrics, self.logger):
                print(f"Early stopping triggered. Best metrics: {early_stopping.get_best_metrics()}")
                break
            if valid_metrics == early_stopping.get_best_metrics():
                os.makedirs(Config.CHECKPOINTS_DIR, exist_ok=True)
                torch.save({"epoch": epoch, "model_state_dict": self.model.state_dict(),
                            "optimizer_state_dict": optimizer.state_dict(), "metrics": valid_metrics,
                            "improvement_rates": early_stopping.get_improvement_rate()},
                           Path(Config.CHECKPOINTS_DIR) / "best_model.pth")
                print("Saved new best model!")
        self.logger.close()
