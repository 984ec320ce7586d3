"""``DomainAdaptationModel`` -- the build's counterpart of reference ``src/models/domain_model.py:4-83``: a segmentation network
and a domain discriminator behind one module, as phase 3 (``UnsupervisedTrainer``) trains them.

Same surface: ``forward(x, domain_adaptation=False)`` (segmentation logits, or ``(logits, domain_pred)``), ``get_features``,
``train`` / ``eval`` / ``to`` over both networks, and ``parameters()`` returning the LIST over both (segmenter first), which is
what the reference hands to its optimizer and to ``clip_grad_norm_``.  ``state_dict`` keys are ``segmentation_model.*`` and
``discriminator.*``.
"""
import torch.nn as nn


class DomainAdaptationModel(nn.Module):
    def __init__(self, segmentation_model, discriminator=None):
        super().__init__()
        self.segmentation_model = segmentation_model
        self.discriminator = discriminator

    @property
    def classes(self):
        return self.segmentation_model.classes

    @property
    def compute_dtype(self):
        return self.segmentation_model.compute_dtype

    def forward(self, x, domain_adaptation=False):
        seg_pred = self.segmentation_model(x)
        if domain_adaptation and self.discriminator is not None:
            return seg_pred, self.discriminator(x)
        return seg_pred

    def get_features(self, x):
        """The deepest encoder feature map (``encoder(x)[-1]`` upstream), or None for a model without an encoder."""
        seg = self.segmentation_model
        if not hasattr(seg, "encoder"):
            return None
        if hasattr(seg, "forward_parts"):
            return seg.forward_parts(x, ("features",))
        return seg.encoder(x)

    def train(self, mode=True):
        self.training = mode
        self.segmentation_model.train(mode)
        if self.discriminator is not None:
            self.discriminator.train(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, device):
        self.segmentation_model = self.segmentation_model.to(device)
        if self.discriminator is not None:
            self.discriminator = self.discriminator.to(device)
        return self

    def parameters(self, recurse=True):
        params = list(self.segmentation_model.parameters())
        if self.discriminator is not None:
            params.extend(self.discriminator.parameters())
        return params
