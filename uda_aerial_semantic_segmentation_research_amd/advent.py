"""Output-space adaptation (AdvEnt, Vu et al., CVPR 2019): what a discriminator that judges the segmenter's *prediction* needs.

The reference's ``AdversarialTrainer`` shows raw images to its discriminator, so its adversarial term never reaches the segmenter
(SURVEY F7/F8).  Here the discriminator sees the weighted self-information maps of the prediction,

    I_c = -p_c log p_c / log C,     p = softmax(logits),     H = sum_c I_c in [0, 1],

so the domain loss trains the whole segmenter through its logits.  A class whose probability is 0 (underflow, a ``-inf`` logit)
contributes exactly 0 and receives a gradient of exactly 0.

* ``self_information(logits, dtype)`` -- differentiable; one HIP pass (csrc/advent.hip) writes the maps into a channel-padded NHWC
  buffer that ``OutputSpaceDiscriminator`` reads in place, and one pass turns the discriminator's input gradient into the logits'.
* ``entropy_map(logits)`` -- ``[B,H,W]`` normalised entropy without a gradient: logging, ranking target frames, ``render``.
* ``OutputSpaceDiscriminator(num_classes, compute_dtype)`` -- ``DomainDiscriminator`` over ``num_classes`` channels that returns
  the gradient with respect to its input.

``losses.EntropyLoss`` is the direct (entropy minimisation) part, ``advent_trainer.AdventTrainer`` wires both into a training step.
"""
import torch

from . import _args as A
from . import kernels as K
from .discriminator import DomainDiscriminator
from .engine import ceil_to, mark_padded_input
from .losses import _check_prediction


def _map_width(classes, dtype):
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"self_information: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
    return ceil_to(classes, 8 if dtype == torch.bfloat16 else 4)


def _padded_map_grad(grad, n, c, h, w, cpad, dtype):
    """The incoming ``[N,C,H,W]`` gradient as a padded NHWC buffer ``[N,H,W,cpad]``: zero-copy when it is already the view of one
    (what ``DomainDiscriminator(input_grad=True)`` returns), otherwise one layout kernel."""
    es = grad.element_size()
    if (grad.dtype == dtype and grad.stride() == (h * w * cpad, 1, w * cpad, cpad) and grad.data_ptr() % 16 == 0
            and grad.untyped_storage().nbytes() - es * grad.storage_offset() >= es * n * h * w * cpad):
        return grad.as_strided((n, h, w, cpad), (h * w * cpad, w * cpad, cpad, 1), grad.storage_offset())
    return K.nchw_to_nhwc(grad.float().contiguous(), cpad, dtype=dtype)


class _SelfInformationFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, dtype):
        n, c, h, w = logits.shape
        buf, ldc = A.padded_nhwc(logits.detach())
        cpad = _map_width(c, dtype)
        maps = torch.empty((n, h, w, cpad), device=logits.device, dtype=dtype)
        K.selfinfo_fwd(buf, n * h * w, c, ldc, maps, cpad)
        mark_padded_input(maps)                       # pad lanes are zeros by construction: a convolution may read it in place
        ctx.save_for_backward(buf)
        ctx.meta = (n, c, h, w, ldc, cpad, dtype)
        ctx.set_materialize_grads(False)              # a consumer without an input gradient hands back None, not a tensor of zeros
        return maps.permute(0, 3, 1, 2)[:, :c]

    @staticmethod
    def backward(ctx, grad):
        if grad is None:                              # e.g. DomainDiscriminator(input_grad=False): nothing flows to the logits
            return None, None
        buf, = ctx.saved_tensors
        n, c, h, w, ldc, cpad, dtype = ctx.meta
        dmaps = _padded_map_grad(grad.detach(), n, c, h, w, cpad, dtype)
        dl = torch.empty((n, h, w, ldc), device=buf.device, dtype=torch.float32)
        K.selfinfo_bwd(buf, dmaps, n * h * w, c, ldc, cpad, dl)
        return dl.permute(0, 3, 1, 2)[:, :c], None


def self_information(logits, dtype=torch.float32):
    """Weighted self-information maps ``-p log p / log C`` of ``softmax(logits)``: ``[B,C,H,W]``, differentiable, ``2 <= C <= 32``.

    The result is a view (strides ``(H*W*cpad, 1, W*cpad, cpad)``) of a padded NHWC buffer of ``dtype`` (fp32: ``cpad = ceil4(C)``,
    bf16: ``ceil8(C)``) whose pad lanes are zeros and which is registered with ``engine.mark_padded_input``: a discriminator of
    that activation type reads it in place.  Do not write into it."""
    _map_width(0, dtype)
    _check_prediction("self_information", logits)
    return A.on_device(logits.device, _SelfInformationFunction.apply, logits, dtype)    # backward: the device's autograd thread


def entropy_map(logits):
    """Per-pixel normalised entropy ``H = -sum_c p_c log p_c / log C`` of ``softmax(logits)``: fp32 ``[B,H,W]`` in ``[0, 1]``, no
    gradient (logging, ranking target frames by confidence; ``render`` takes the range as it is)."""
    _check_prediction("entropy_map", logits)
    n, c, h, w = logits.shape
    dev = logits.device
    with torch.no_grad():
        buf, ldc = A.padded_nhwc(logits.detach())
        out = torch.empty((n, h, w), device=dev, dtype=torch.float32)
        A.on_device(dev, K.entropy_loss, buf, n * h * w, c, ldc, "entropy", torch.empty(K.seg_partials(), device=dev, dtype=torch.float64),
                    torch.empty((), device=dev, dtype=torch.float32), None, out)
    return out


class OutputSpaceDiscriminator(DomainDiscriminator):
    """The domain classifier of output-space adaptation: ``DomainDiscriminator`` over ``num_classes`` self-information channels,
    returning the gradient with respect to its input (``input_grad=True``).  Same layers, same ``state_dict`` keys."""

    def __init__(self, num_classes, compute_dtype=torch.float32):
        super().__init__(input_channels=num_classes, compute_dtype=compute_dtype, input_grad=True)
