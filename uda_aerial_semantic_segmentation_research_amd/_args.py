"""The host-side argument rules of the device feature modules, stated once: scalar ranges, tensor operands, the device guard of a
launch, eval mode, constant device tables and lazily allocated device state.  Imports no feature module.

Tensor rules check the VALUE first, then the PLACE: a non-tensor, a wrong dtype, rank or shape or an empty tensor is a
``ValueError`` on any device; a well-formed tensor that is not on a GPU is a ``RuntimeError`` ("no CPU path in this build"); two
well-formed tensors on different GPUs are a ``ValueError`` naming both.  Messages read ``"{who}: {name} must be ..., got ..."``.
"""
import contextlib

import numpy as np
import torch

from . import _lib
from . import kernels as K

NO_CPU = "(no CPU path in this build)"


# ----------------------------------------------------------------------------------------------------------------- scalars
def int_in(who, name, v, lo, hi=None, none_ok=False):
    """``int(v)`` of an ``int`` or ``np.integer`` (never a ``bool``) in ``lo..hi`` (``hi=None``: no upper bound)."""
    if v is None and none_ok:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{who}: {name} must be an int {f'>= {lo}' if hi is None else f'in {lo}..{hi}'}"
                         f"{' or None' if none_ok else ''}, got {v!r}")
    return int(v)


def number(who, name, v, lo=-np.inf, hi=np.inf, lo_open=False):
    """``float(v)`` of a finite number in ``[lo, hi]`` (``lo_open``: ``(lo, hi]``)."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = np.nan
    if not np.isfinite(f) or f < lo or f > hi or (lo_open and f == lo):
        raise ValueError(f"{who}: {name} must be a finite number in {'(' if lo_open else '['}{lo}, {hi}], got {v!r}")
    return f


def pair(who, name, v, lo, hi, lo_open=False):
    """``(a, b)`` as floats with ``lo <= a <= b <= hi`` (``lo_open``: ``lo < a``)."""
    try:
        a, b = (float(x) for x in v)
    except (TypeError, ValueError):
        a = b = np.nan
    if not lo <= a <= b <= hi or (lo_open and a == lo):
        raise ValueError(f"{who}: {name} must be a pair (lo, hi) with {lo} {'<' if lo_open else '<='} lo <= hi <= {hi}, got {v!r}")
    return a, b


def choice(who, name, v, allowed):
    """``v`` if it is one of ``allowed`` (a ``bool`` never is)."""
    if isinstance(v, bool) or v not in tuple(allowed):
        raise ValueError(f"{who}: {name} must be one of {tuple(allowed)}, got {v!r}")
    return v


# ----------------------------------------------------------------------------------------------------------------- tensors
def _bad(who, name, t, want):
    return ValueError(f"{who}: {name} must be {want}, got {getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")


def same_gpu(who, **tensors):
    """The place of well-formed tensors (``None`` is skipped): every one on ONE GPU -> that device."""
    dev = first = None
    for name, t in tensors.items():
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(f"{who}: {name} must live on the GPU {NO_CPU}")
        if dev is None:
            dev, first = t.device, name
        elif t.device != dev:
            raise ValueError(f"{who}: {first} is on {dev}, {name} on {t.device}")
    return dev


def label_maps(who, labels, name="labels"):
    """A label map, uint8 or int64 ``[N,H,W]`` or ``[H,W]``, non-empty, on the GPU -> (contiguous ``[N,H,W]``, single)."""
    if not (torch.is_tensor(labels) and labels.dtype in (torch.uint8, torch.int64) and labels.dim() in (2, 3) and labels.numel() > 0):
        raise _bad(who, name, labels, "a non-empty uint8 or int64 [N,H,W] (or [H,W]) tensor")
    same_gpu(who, **{name: labels})
    single = labels.dim() == 2
    return (labels[None] if single else labels).contiguous(), single


def padded_nhwc(logits):
    """[N,C,H,W] logits -> (tensor whose storage is the padded NHWC buffer [N,H,W,ldc], ldc).  Zero-copy when the
    logits come from ``Unet.forward``; otherwise one layout kernel, launched with the logits' device current."""
    n, c, h, w = logits.shape
    ldc = (c + 3) // 4 * 4
    if (logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.stride(3) == ldc and logits.stride(2) == ldc * w
            and logits.stride(0) == ldc * w * h
            and logits.untyped_storage().nbytes() - 4 * logits.storage_offset() >= 4 * n * h * w * ldc):
        return logits.as_strided((n, h, w, ldc), (h * w * ldc, w * ldc, ldc, 1), logits.storage_offset()), ldc
    x = logits.float().contiguous()          # a CPU tensor goes straight to the kernel's own refusal (and to a host test's stub)
    return (on_device(x.device, K.nchw_to_nhwc, x, ldc) if x.is_cuda else K.nchw_to_nhwc(x, ldc)), ldc


def logits_nhwc(logits):
    """[N,C,H,W] fp32 logits -> (padded NHWC buffer [N,H,W,ldc], ldc): zero-copy for ``Unet.forward``'s output (whose ldc is
    the head's padded width), ``padded_nhwc`` otherwise."""
    n, c, h, w = logits.shape
    ldc = logits.stride(3)
    if (logits.dtype == torch.float32 and logits.stride(1) == 1 and ldc % 4 == 0 and ldc >= c and logits.stride(2) == ldc * w
            and logits.stride(0) == ldc * w * h
            and logits.untyped_storage().nbytes() - 4 * logits.storage_offset() >= 4 * n * h * w * ldc):
        return logits.as_strided((n, h, w, ldc), (h * w * ldc, w * ldc, ldc, 1), logits.storage_offset()), ldc
    return padded_nhwc(logits)


def scores_shape(who, scores, classes=None, name="scores", max_classes=32):
    """The value of scores ``[N,C,H,W]``: fp32 or bf16, ``1 <= C <= max_classes`` (``C == classes`` when given), ``N, H, W >= 1``,
    ``H * W < 2^31`` -> ``(n, c, h, w)``."""
    ok = torch.is_tensor(scores) and scores.dim() == 4 and scores.dtype in (torch.float32, torch.bfloat16)
    n, c, h, w = scores.shape if ok else (0, 0, 0, 0)
    if not (ok and 1 <= c <= max_classes and classes in (None, c) and min(n, h, w) >= 1 and h * w < 2 ** 31):
        form = f"[N,C,H,W] tensor with num_classes = C in 1..{max_classes}," if classes is None else f"[N,{classes},H,W] tensor with"
        raise _bad(who, name, scores, f"a float32 or bfloat16 {form} N, H, W >= 1 and H * W < 2^31")
    return n, c, h, w


def scores_nchw(who, scores, classes=None, name="scores", max_classes=32):
    """``scores_shape``, then the place (on the GPU) -> ``(buf, ld, n, c, h, w)`` with ``padded_nhwc``'s buffer of the detached
    scores."""
    n, c, h, w = scores_shape(who, scores, classes, name, max_classes)
    same_gpu(who, **{name: scores})
    buf, ld = padded_nhwc(scores.detach())
    return buf, ld, n, c, h, w


def flat_targets(who, masks, pixels, name="masks"):
    """Masks ``[N,H,W]`` or ``[N,1,H,W]`` of ``pixels`` elements -> contiguous int64 ``[pixels]``."""
    if not (torch.is_tensor(masks) and masks.numel() == pixels):
        raise _bad(who, name, masks, f"a [N,H,W] or [N,1,H,W] tensor of {pixels} elements matching the scores")
    tgt = masks.reshape(-1)
    return (tgt if tgt.dtype == torch.int64 else tgt.long()).contiguous()


def frames_u8(who, frames, shape=None, name="frames", below_2_31=False):
    """uint8 frames ``[N,H,W,3]`` with ``N, H, W >= 1`` (``(N, H, W) == shape`` when given; ``below_2_31``: ``N*H*W < 2^31``) ->
    ``(n, h, w)``.  The value alone: the caller moves host frames or asks ``same_gpu``."""
    ok = torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
    n, h, w = frames.shape[:3] if ok else (0, 0, 0)
    if not (ok and min(n, h, w) >= 1 and (shape is None or tuple(shape) == (n, h, w)) and not (below_2_31 and n * h * w >= 2 ** 31)):
        raise _bad(who, name, frames, f"a uint8 {'[N,H,W,3]' if shape is None else list(shape) + [3]} tensor with N, H, W >= 1"
                                      f"{' and N*H*W < 2^31' if below_2_31 else ''}")
    return n, h, w


def out_tensor(who, name, out, shape, dtype, dev, contiguous=False):
    """``out``, allocated when ``None``; otherwise a tensor of exactly this dtype, shape and device (``contiguous``: and dense)."""
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=dev)
    if (not torch.is_tensor(out) or out.dtype != dtype or tuple(out.shape) != tuple(shape) or out.device != dev
            or (contiguous and not out.is_contiguous())):
        raise _bad(who, name, out, f"a {'contiguous ' if contiguous else ''}{dtype} {list(shape)} tensor on {dev}")
    return out


def counts_tensor(who, name, counts, shape, dev):
    """An optional table of counters a kernel accumulates into: ``None`` passes, otherwise int64 of exactly this shape on ``dev``."""
    return None if counts is None else out_tensor(who, name, counts, shape, torch.int64, dev)


# --------------------------------------------------------------------------------------------------------- device and mode
def on_device(dev, fn, *args):
    """``fn(*args)`` with ``dev`` current: a launch goes to the CURRENT device's stream, so the tensors' device is made current."""
    if dev.index == torch.cuda.current_device():
        return fn(*args)
    with torch.cuda.device(dev):
        return fn(*args)


def model_device(model, who, max_classes=None):
    """The GPU a model's parameters live on; a model on the CPU raises, and so does one of more than ``max_classes`` classes when
    the caller gives its bound (one pixel's class row lives in registers)."""
    p = next(iter(model.parameters()), None)
    if p is None or p.device.type != "cuda":
        raise RuntimeError(f"{who}: the model must live on the GPU {NO_CPU}")
    classes = getattr(model, "classes", None)
    if classes is not None and max_classes is not None and not 1 <= classes <= max_classes:
        raise ValueError(f"{who}: classes must lie in 1..{max_classes}, got {classes}")
    return p.device


def current_gpu():
    """The current GPU as a device, after ``_lib.require_gpu()``."""
    _lib.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


@contextlib.contextmanager
def eval_mode(model):
    """``model.eval()`` inside; the training flag it had is restored on the way out, by an exception too."""
    was = model.training
    model.eval()
    try:
        yield model
    finally:
        model.train(was)


CONST_TABLES = 64
_CONST = {}


def const_table(space, key, make, dev):
    """The device copy of a small constant table, kept per ``(space, key, device)``: ``make()`` gives a numpy array or a tuple of
    them and runs once.  At most ``CONST_TABLES`` are kept; a full cache is emptied.  The upload is a copy from pageable host
    memory, which returns only after the bytes are on the device, so a kept table is complete whatever stream reads it later; it
    is never written again."""
    key = (space, key, str(dev))
    t = _CONST.get(key)
    if t is None:
        if len(_CONST) >= CONST_TABLES:
            _CONST.clear()
        arr = make()
        t = _CONST[key] = (tuple(torch.from_numpy(a).to(dev) for a in arr) if isinstance(arr, tuple)
                           else torch.from_numpy(arr).to(dev))
    return t


class DeviceState:
    """Device state allocated on first use by the class's own ``_allocate(device)`` and bound to that GPU from then on."""
    device = _home = None

    def _ensure(self, device=None):
        if self._home is not None and (device is None or device == self._home):
            return self
        device = torch.device(device or self.device or "cuda")
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._home is None:
            if device.type != "cuda":
                raise RuntimeError(f"{type(self).__name__}: tensors must live on the GPU {NO_CPU}")
            self._allocate(device)
            self.device = self._home = device
        elif device != self._home:
            raise ValueError(f"{type(self).__name__}: the state lives on {self._home}, the tensors on {device}")
        return self
