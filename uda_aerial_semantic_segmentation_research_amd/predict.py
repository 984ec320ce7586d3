"""Prediction -- mirror of reference ``src/models/predict.py``: ``predict_mask`` (:70-111) and ``predict_batch`` (:113-130),
plus ``predict_large``: the label map of one frame of any size, by tiled, blended inference with optional test-time
augmentation (TTA) over the dihedral group D4.

The reference resizes a whole frame to the model's input size (``Resize(Config.IMAGE_SIZE)``); aerial frames are thousands of
pixels on a side and the labels are per pixel, so ``predict_large`` runs the model on a regular grid of overlapping tiles at
full resolution and blends their class probabilities back with a window.  The passes around the eval forward are HIP kernels
(csrc/predict.hip): the tile gather (crop + reflect padding + D4 view + ``A.Normalize``), the blend into a per-pixel
accumulator, the final division + argmax, and predict_mask's sigmoid threshold.  No CPU path.

Tile grid, per axis of length ``L`` with requested tile ``tile`` (a multiple of 32) and ``overlap`` in [0, 0.5]:
effective tile ``t = min(tile, ceil32(L))``, stride ``s = t - round(overlap * t)``, origins ``[0]`` if ``L <= t`` else
``o_i = min(i*s, L - t)`` for ``i = 0 .. ceil((L - t) / s)`` -- the last tile is flush with the edge.  Tiles run raster,
row-major.  Pixels outside the frame (only when ``L < t``) are mirrored as ``numpy.pad(mode="reflect")``.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _args as A
from . import _lib
from . import kernels as K
from .config import Config
from .data import FLIP_COLS, FLIP_ROWS, IMAGENET_MEAN, IMAGENET_STD, TRANSPOSE, normalize_constants, prepare_batch
from .engine import ceil4, mark_padded_input

MAX_CLASSES = 32                                   # as the loss kernels: one pixel's class row lives in registers
VIEWS = {None: (0,), "flips": (0, 2, 4, 6), "d4": tuple(range(8))}     # D4 codes per TTA mode (data.py's convention)
WINDOWS = ("gaussian", "uniform")

Grid = namedtuple("Grid", "h w th tw rows cols sy sx oy ox")


def _ceil32(n):
    return (n + 31) // 32 * 32


def plan_axis(length, tile, overlap):
    """(effective tile t, stride s, origins) of one frame axis (module docstring)."""
    if not isinstance(length, (int, np.integer)) or length < 1:
        raise ValueError(f"frame side must be >= 1, got {length}")
    if not isinstance(tile, (int, np.integer)) or tile < 32 or tile % 32:
        raise ValueError(f"tile sides must be positive multiples of 32, got {tile}")
    if not 0.0 <= overlap <= 0.5:
        raise ValueError(f"overlap must lie in [0, 0.5], got {overlap}")
    t = min(int(tile), _ceil32(int(length)))
    s = t - int(round(overlap * t))
    if length <= t:
        return t, s, [0]
    n = -(-(length - t) // s) + 1
    return t, s, [min(i * s, length - t) for i in range(n)]


def plan_grid(h, w, tile=512, overlap=0.25):
    """The tile grid of an ``h x w`` frame; ``tile`` is an int or ``(th, tw)``."""
    th, tw = (tile, tile) if isinstance(tile, (int, np.integer)) else tuple(tile)
    th, sy, oy = plan_axis(h, th, overlap)
    tw, sx, ox = plan_axis(w, tw, overlap)
    return Grid(h, w, th, tw, len(oy), len(ox), sy, sx, oy, ox)


def _grid_args(g):
    return (g.h, g.w, g.th, g.tw, g.rows, g.cols, g.sy, g.sx)


def window_vector(t, window="gaussian"):
    """fp32 blend weights of one tile axis.  ``"gaussian"``: exp(-0.5*((i-(t-1)/2)/(t/8))^2) in float64, divided by its maximum,
    clamped to >= 1e-3, rounded to fp32; ``"uniform"``: ones.  The tile weight is ``wy[ty] * wx[tx]`` in fp32."""
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
    if window == "uniform":
        return np.ones(t, dtype=np.float32)
    i = np.arange(t, dtype=np.float64)
    g = np.exp(-0.5 * ((i - (t - 1) / 2.0) / (t / 8.0)) ** 2)
    return np.maximum(g / g.max(), 1e-3).astype(np.float32)


def apply_view(code, y, x, th, tw):
    """Tile pixel shown at pixel (y, x) of view ``code`` of a ``th x tw`` tile (``data._apply_code`` for non-square tiles)."""
    if code & FLIP_ROWS:
        y = th - 1 - y
    if code & FLIP_COLS:
        x = tw - 1 - x
    return (x, y) if code & TRANSPOSE else (y, x)


def inverse_view(code, ty, tx, th, tw):
    """Pixel of view ``code`` (i.e. of the model's output for it) that holds tile pixel (ty, tx): the blend's read."""
    y, x = (tx, ty) if code & TRANSPOSE else (ty, tx)
    return (th - 1 - y if code & FLIP_ROWS else y), (tw - 1 - x if code & FLIP_COLS else x)


def view_mask(codes):
    return sum(1 << c for c in codes)


def predict_batch(model, images, device="cuda"):
    """Reference ``predict.py:113-130``: ``model.eval()`` (left so), then under ``no_grad`` the argmax over classes of
    ``model(images)`` -> numpy int64 ``[B,H,W]``, ties to the first maximal index as ``torch.argmax``.  ``images`` is any
    ``[B,3,H,W]`` tensor (the view ``data.prepare_batch`` returns included); the argmax is one HIP kernel reading the padded
    NHWC logits in place."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("predict_batch: device must be a GPU (no CPU path in this build)")
    _lib.require_gpu()
    A.model_device(model, "predict_batch", MAX_CLASSES)
    model.eval()
    with torch.no_grad():
        logits = model(images.to(dev))
        n, c, h, w = logits.shape
        buf, ldc = A.logits_nhwc(logits)
        labels = torch.empty((n, h, w), dtype=torch.int64, device=buf.device)
        K.predict_finish(buf, None, n * h * w, c, ldc, labels)
        return labels.cpu().numpy()


def predict_mask(model, img, device=None, resize=False):
    """Reference ``predict.py:70-111``, quirk included: ``(sigmoid(logits) > 0.5)`` as float 0/1, ``.squeeze()``d, as numpy
    (``[C,H,W]`` for one image) -- multi-class thresholding, not an argmax.

    * A tensor (``[3,H,W]`` or ``[1,3,H,W]``, normalised) is used as is, as the reference's tensor branch does; ``resize``
      does not apply to it (``ingest.resize_normalized`` makes such a tensor from a uint8 frame).
    * A numpy uint8 ``[H,W,3]`` RGB image (or a PIL image) is normalised by ``data.prepare_batch``: ``A.Normalize``'s fp32
      ``(x - 255*mean) * (1 / (255*std))``, where the reference's ``ToTensor`` + ``Normalize`` computes
      ``(x / 255 - mean) / std`` -- the same up to one fp32 rounding.  The reference then resizes to ``Config.IMAGE_SIZE``;
      that is the identity only at that size, so any other size raises ``ValueError`` (use ``predict_large``) -- unless
      ``resize=True``: then a frame of any size goes through ``ingest.resize_normalized`` (antialiased bilinear + the same
      ``A.Normalize``, csrc/resize.hip) to ``Config.IMAGE_SIZE`` on the model's device, and the result stays at the model's size,
      as the reference's does.
    The threshold is one HIP kernel writing the NCHW float output."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("predict_mask: device must be a GPU (no CPU path in this build)")
    _lib.require_gpu()
    A.model_device(model, "predict_mask", MAX_CLASSES)
    model.eval()
    try:
        from PIL import Image
        if isinstance(img, Image.Image):
            img = np.asarray(img.convert("RGB"))
    except ImportError:
        pass
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"predict_mask: numpy images must be uint8 [H,W,3] RGB, got {img.dtype} {img.shape}")
        if resize:
            from .ingest import frame_for_model
            x = frame_for_model(model, img)
        elif tuple(img.shape[:2]) != tuple(Config.IMAGE_SIZE):
            raise ValueError(f"predict_mask: image is {img.shape[0]}x{img.shape[1]}, the model size is "
                             f"{Config.IMAGE_SIZE[0]}x{Config.IMAGE_SIZE[1]}; the reference's Resize is not reproduced here -- "
                             f"use predict_large for frames of other sizes")
        else:
            x, _ = prepare_batch(torch.from_numpy(np.ascontiguousarray(img))[None], dtype=getattr(model, "compute_dtype",
                                                                                                  torch.float32))
    elif torch.is_tensor(img):
        x = (img.unsqueeze(0) if img.dim() == 3 else img).to(dev)
    else:
        raise TypeError(f"predict_mask: expected a tensor, a numpy uint8 image or a PIL image, got {type(img).__name__}")
    with torch.no_grad():
        logits = model(x)
        n, c, h, w = logits.shape
        buf, ldc = A.logits_nhwc(logits)
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=buf.device)
        K.predict_threshold(buf, n, h * w, c, ldc, out)
    return out.squeeze().cpu().numpy()


def predict_large(model, image, tile=512, overlap=0.25, batch_size=8, tta=None, window="gaussian", return_probs=False,
                  mean=IMAGENET_MEAN, std=IMAGENET_STD, max_pixel_value=255.0, _events=None):
    """Label map of one frame of any size: int64 ``[H,W]`` on the device (and, with ``return_probs``, the blended class
    probabilities as a ``[1,C,H,W]``-shaped fp32 view of a padded NHWC buffer with ``ldc = ceil4(C)`` -- the layout of
    ``Unet.forward``'s logits, so ``metrics.segmentation_metrics(probs, mask[None], C)`` takes it without a copy).

    ``image``: uint8 ``[H,W,3]`` RGB, numpy or a tensor, on the host (copied once) or the device.  The tile grid and edge
    padding are the module docstring's.  ``tta``: None (code 0), ``"flips"`` (the four non-transposing D4 codes) or ``"d4"``
    (all eight; square tiles only).  View ``c`` of a tile feeds the model the tile under code ``c`` exactly as
    ``data.prepare_batch`` would; the blend maps the output back.  Per pixel, a tile adds ``w(ty,tx) * sum_v softmax(logits_v)``
    to an accumulator and ``w * V`` to its weight, one tile at a time in raster order (no atomics: bit-identical for every
    ``batch_size`` and across calls); ``probs = acc / wsum`` and ``labels = argmax(probs)`` (first maximum on ties).
    ``window``: ``"gaussian"`` or ``"uniform"`` (``window_vector``).  One forward takes ``max(1, batch_size // V)`` tiles
    times ``V`` views; the model runs in eval mode (left so), fp32 or bf16 ``compute_dtype``, and reads the gathered tiles in
    place.

    Memory: the accumulator is ``H*W*(ceil4(C)+1)*4`` bytes (about 2.4 GB for a 4000 x 6000 frame at 23 classes), plus the
    uint8 frame, the labels (8 bytes per pixel) and one batch of tiles, logits and activations."""
    if tta not in VIEWS:
        raise ValueError(f"tta must be None, 'flips' or 'd4', got {tta!r}")
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise ValueError(f"predict_large: image must be uint8 [H,W,3] RGB, got {image.dtype} {image.shape}")
        image = torch.from_numpy(np.ascontiguousarray(image))
    if not torch.is_tensor(image) or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise ValueError(f"predict_large: image must be uint8 [H,W,3] RGB, got "
                         f"{getattr(image, 'dtype', type(image).__name__)} {tuple(getattr(image, 'shape', ()))}")
    h, w = int(image.shape[0]), int(image.shape[1])
    g = plan_grid(h, w, tile, overlap)
    codes = VIEWS[tta]
    if tta == "d4" and g.th != g.tw:
        raise ValueError(f"tta='d4' needs square tiles, got {g.th}x{g.tw} (tiles are clamped to ceil32 of each frame side)")
    _lib.require_gpu()
    dev = A.model_device(model, "predict_large", MAX_CLASSES)
    classes = model.classes
    nv, mask = len(codes), view_mask(codes)
    per_fwd = max(1, int(batch_size) // nv)
    dtype = getattr(model, "compute_dtype", torch.float32)
    cpad = model.encoder.conv1.cin_p
    ldp = ceil4(classes)
    img = image.to(dev, non_blocking=True).contiguous()
    acc = torch.zeros(h * w * ldp, dtype=torch.float32, device=dev)
    wsum = torch.zeros(h * w, dtype=torch.float32, device=dev)
    win_y = torch.from_numpy(window_vector(g.th, window)).to(dev)
    win_x = torch.from_numpy(window_vector(g.tw, window)).to(dev)
    m255, r255 = normalize_constants(mean, std, max_pixel_value)
    xbuf = torch.empty((min(per_fwd, g.rows * g.cols) * nv, g.th, g.tw, cpad), dtype=dtype, device=dev)
    mark_padded_input(xbuf)                  # the stem reads the gathered tiles in place (Unet._padded_input_view)
    args = _grid_args(g)

    def mark(kind):                          # tools/bench_predict.py: device time of each phase (interval to the next mark)
        if _events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            _events.append((kind, e))

    model.eval()
    n_tiles = g.rows * g.cols
    with torch.no_grad():
        for first in range(0, n_tiles, per_fwd):
            tiles = min(per_fwd, n_tiles - first)
            xb = xbuf[: tiles * nv]
            mark("gather")
            K.predict_gather_u8(img, args, first, tiles, mask, m255, r255, xb)
            mark("forward")
            logits = model(xb.permute(0, 3, 1, 2)[:, :3])
            mark("blend")
            lbuf, ldc = A.logits_nhwc(logits)
            K.predict_blend(lbuf, ldc, args, first, tiles, mask, classes, win_y, win_x, acc, ldp, wsum)
            mark("end")
        labels = torch.empty((h, w), dtype=torch.int64, device=dev)
        mark("finish")
        K.predict_finish(acc, wsum, h * w, classes, ldp, labels)
        mark("end")
    if not return_probs:
        return labels
    probs = acc.view(1, h, w, ldp).permute(0, 3, 1, 2)[:, :classes]
    return labels, probs


def accumulator_bytes(h, w, classes):
    """Device bytes of predict_large's accumulator (probabilities + weights) for an ``h x w`` frame."""
    return h * w * (ceil4(classes) + 1) * 4


__all__ = ["predict_batch", "predict_mask", "predict_large", "plan_axis", "plan_grid", "window_vector", "apply_view",
           "inverse_view", "accumulator_bytes", "VIEWS"]
