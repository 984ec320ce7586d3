"""Rendering of predictions on the device: colour masks, overlays on the frame, error maps, class outlines and per-image class
counts -- what the reference does on the host after every prediction (``predict.py``: ``create_colored_mask``, ``create_overlay``
and the ``np.unique`` class distribution of ``test_model``; ``train.py``: ``_log_predictions`` and the ``true_colored`` /
``pred_colored`` loops).  Labels in, uint8 RGB pictures and int64 counts out, ONE HIP pass (``udaseg_render_u8``,
csrc/render.hip), nothing on the host: a 4000 x 6000 label map from ``predict_large`` is 192 MB of int64 that never has to leave
the GPU to be looked at.

The rule (part of the public contract; ``tests/_render_ref.py`` is its numpy mirror and the GPU tests compare bit for bit).
Per pixel of an image ``[H][W]``:

    label ``L``     uint8 or int64 labels; an int64 value outside ``[0, 255]`` reads as 255.
    colour ``c``    ``table[L]``; ``table`` is uint8 ``[256][3]``: the palette's colours for ``0 .. classes-1``, ``void_color``
                    for every other entry (``palette_table``).
    base ``b``      a uint8 frame ``[N,H,W,3]``; or the model input as ``data.prepare_batch`` / ``train_batch`` / ``strong_views``
                    return it (padded NHWC, fp32 with 4 or bf16 with 8 channels per pixel), de-normalised per channel as
                    ``clip(round_half_even(x * (std*255) + mean*255), 0, 255)`` in fp32 (one multiply, one add, NaN -> 0); or none.
    category ``k``  3: a truth label is given and is void (``== ignore_index`` or ``>= classes``); else 2: a truth label is given
                    and equals ``L``; else 1: ``L`` is void (``L >= classes``); else 0.
    blend           ``out = (b*(256 - a[k]) + c*a[k] + 128) >> 8`` per channel in integers, ``a[k] = round_half_even(alpha_k * 256)``
                    in ``[0, 256]``: within one level of ``b(1-alpha) + c*alpha`` (0.5 from the final rounding, 255/512 from the
                    rounding of alpha), ``a = 0`` returns ``b`` and ``a = 256`` returns ``c`` exactly.  Without a base, ``out = c``.
    outline         optional: a pixel whose label differs from its left, right, upper or lower neighbour inside the same image
                    gets ``outline`` (an RGB colour) instead; the frame's edge is no outline.
    counts          optional int64 ``[N,256]`` histogram of ``L`` per image and, with truth, ``[N,3]`` agree / differ / truth void.
                    Both ACCUMULATE when the caller hands in its own tensors, like the project's other count outputs.

``[H,W]`` labels (and ``[H,W,3]`` frames) are taken as ``N = 1`` and the picture comes back without the batch axis.  CPU tensors
raise: there is no CPU path in this build.
"""
import csv

import numpy as np
import torch

from . import _args as A
from . import kernels as K
from .data import IMAGENET_MEAN, IMAGENET_STD

VOID_COLOR = (0, 0, 0)
OUTLINE_WHITE = (255, 255, 255)


# --------------------------------------------------------------------------------------------------------------- host side
def default_palette(n=256):
    """uint8 ``[n,3]``: the bit-reversal colour map of the PASCAL VOC label images.  The three low bits of the class number go to
    the top bit of r, g, b, the next three bits to the next lower bit, and so on: 0 is black, 1 (128,0,0), 2 (0,128,0), ... --
    256 distinct colours, neighbours in number far apart in colour."""
    if not isinstance(n, (int, np.integer)) or not 1 <= n <= 256:
        raise ValueError(f"default_palette: n must lie in 1..256, got {n}")
    pal = np.zeros((int(n), 3), dtype=np.uint8)
    for i in range(int(n)):
        c, rgb = i, [0, 0, 0]
        for j in range(8):
            for ch in range(3):
                rgb[ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
        pal[i] = rgb
    return pal


def load_palette(path):
    """``(names, colours)`` of a ``class_dict_seg.csv``-style file: a header line, then ``name, r, g, b`` per class.
    ``colours`` is uint8 ``[classes,3]``."""
    names, colours = [], []
    with open(path, newline="") as fh:
        rows = [r for r in csv.reader(fh, skipinitialspace=True) if r and any(f.strip() for f in r)]
    if not rows:
        raise ValueError(f"load_palette: {path} is empty")
    try:
        [int(v) for v in rows[0][1:4]]
    except ValueError:
        rows = rows[1:]                                            # the header line
    for r in rows:
        if len(r) < 4:
            raise ValueError(f"load_palette: a row needs name, r, g, b; got {r}")
        rgb = [int(v) for v in r[1:4]]
        if not all(0 <= v <= 255 for v in rgb):
            raise ValueError(f"load_palette: colour out of range in {r}")
        names.append(r[0].strip())
        colours.append(rgb)
    if not 1 <= len(names) <= 256:
        raise ValueError(f"load_palette: 1..256 classes are needed, {path} has {len(names)}")
    return names, np.asarray(colours, dtype=np.uint8)


def _color(who, rgb):
    v = np.asarray(rgb)
    if v.shape != (3,) or not np.all((v >= 0) & (v <= 255)) or not np.all(v == np.floor(v)):
        raise ValueError(f"{who} must be an (r, g, b) of integers in 0..255, got {rgb}")
    return tuple(int(x) for x in v)


def table_array(colours, classes, void_color=VOID_COLOR):
    """The host form of ``palette_table``: numpy uint8 ``[256,3]``."""
    col = np.asarray(colours)
    if col.ndim != 2 or col.shape[1] != 3 or not np.all((col >= 0) & (col <= 255)):
        raise ValueError(f"palette colours must be [K,3] values in 0..255, got shape {col.shape}")
    if not isinstance(classes, (int, np.integer)) or not 1 <= classes <= 256:
        raise ValueError(f"classes must lie in 1..256, got {classes}")
    if classes > col.shape[0]:
        raise ValueError(f"the palette has {col.shape[0]} colours, {classes} classes need as many")
    t = np.empty((256, 3), dtype=np.uint8)
    t[:] = np.asarray(_color("void_color", void_color), dtype=np.uint8)
    t[:classes] = col[:classes].astype(np.uint8)
    return t


def palette_table(colours, classes, void_color=VOID_COLOR, device=None):
    """The uint8 ``[256,3]`` device table of a palette: ``colours[L]`` for ``L < classes``, ``void_color`` for every other entry.
    ``device``: None is the current GPU."""
    t = torch.from_numpy(table_array(colours, classes, void_color))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return t.to(dev)


def alpha_level(alpha):
    """``round_half_even(alpha * 256)``: the integer weight in ``[0, 256]`` of an opacity in ``[0, 1]``."""
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"an opacity in [0, 1] is needed, got {alpha}")
    return int(np.rint(np.float64(alpha) * 256.0))


def denorm_constants(mean=IMAGENET_MEAN, std=IMAGENET_STD, max_pixel_value=255.0):
    """Six fp32 values (as floats): ``std * max_pixel_value`` then ``mean * max_pixel_value``, each factor rounded to fp32 first and
    the product rounded to fp32 -- the inverse of ``data.normalize_constants``."""
    mx = np.float32(max_pixel_value)
    return [float(np.float32(np.float32(s) * mx)) for s in std] + [float(np.float32(np.float32(m) * mx)) for m in mean]


_DENORM = {}


def _denorm_cached(mean, std):
    d = _DENORM.get((mean, std))
    if d is None:
        if len(_DENORM) > 64:
            _DENORM.clear()
        d = _DENORM[(mean, std)] = tuple(denorm_constants(mean, std))
    return d


def class_shares(counts):
    """float64 shares of a count table (numpy or tensor, last axis = labels): ``counts / counts.sum(-1)``, zeros for an empty row."""
    if torch.is_tensor(counts):
        counts = counts.detach().cpu().numpy()
    c = np.asarray(counts).astype(np.float64)
    tot = c.sum(axis=-1, keepdims=True)
    return np.divide(c, tot, out=np.zeros_like(c), where=tot > 0)


def format_stats(counts, names):
    """The class-distribution block of the reference's ``test_model``: one ``"  name: 12.34%"`` line per class PRESENT, in label
    order.  ``counts``: ``[256]`` (or ``[N,256]``, summed over the images); a label without a name prints as ``class <L>``."""
    if torch.is_tensor(counts):
        counts = counts.detach().cpu().numpy()
    c = np.asarray(counts).astype(np.int64)
    if c.ndim == 2:
        c = c.sum(axis=0)
    if c.ndim != 1:
        raise ValueError(f"format_stats: counts must be [L] or [N,L], got shape {c.shape}")
    total = int(c.sum())
    lines = []
    for lab in np.nonzero(c)[0]:
        name = names[lab] if lab < len(names) else f"class {int(lab)}"
        lines.append(f"  {name}: {int(c[lab]) / total * 100:.2f}%\n")
    return "".join(lines)


# ------------------------------------------------------------------------------------------------------------- device side
def _table_for(palette, classes, void_color, dev):
    """(device table, classes) of the ``palette`` argument: None (the default palette), ``[K,3]`` colours, or a ready uint8
    ``[256,3]`` device table (then ``classes`` must be given)."""
    if torch.is_tensor(palette) and palette.is_cuda:
        if palette.dtype != torch.uint8 or tuple(palette.shape) != (256, 3):
            raise ValueError(f"a device palette must be the uint8 [256,3] table of palette_table, got {palette.dtype} {tuple(palette.shape)}")
        if classes is None:
            raise ValueError("classes must be given with a ready device table")
        return palette, A.int_in("palette", "classes", classes, 1, 256)
    col = default_palette() if palette is None else (palette.numpy() if torch.is_tensor(palette) else np.asarray(palette))
    if classes is None:
        classes = int(col.shape[0]) if col.ndim == 2 else 0
    arr = table_array(col, classes, void_color)
    return A.const_table("render", arr.tobytes(), lambda: arr, dev), int(classes)


def _base(who, frames, n, h, w, single):
    """-> the contiguous base operand: uint8 [N,H,W,3], or the padded fp32 [N,H,W,4] / bf16 [N,H,W,8] buffer behind a model input
    (the ``[N,3,H,W]``-shaped view ``data.prepare_batch`` hands out is taken in place; any other ``[N,3,H,W]`` / ``[N,H,W,C]``
    float tensor is copied into a padded buffer)."""
    if not torch.is_tensor(frames):
        raise ValueError(f"{who}: frames must be a tensor, got {type(frames).__name__}")
    if frames.device.type != "cuda":
        raise RuntimeError(f"{who}: frames must live on the GPU (no CPU path in this build)")
    if frames.dim() == 3 and single:
        frames = frames[None]
    if frames.dtype == torch.uint8:
        if tuple(frames.shape) != (n, h, w, 3):
            raise ValueError(f"{who}: a uint8 frame must be [{n},{h},{w},3], got {tuple(frames.shape)}")
        return frames.contiguous()
    if frames.dtype not in (torch.float32, torch.bfloat16) or frames.dim() != 4:
        raise ValueError(f"{who}: frames must be uint8 [N,H,W,3] or an fp32 / bf16 model input, got {frames.dtype} {tuple(frames.shape)}")
    cpad = 4 if frames.dtype == torch.float32 else 8
    if tuple(frames.shape) == (n, h, w, cpad):
        x = frames.contiguous()
    elif tuple(frames.shape) == (n, 3, h, w):
        if (frames.stride() == (h * w * cpad, 1, w * cpad, cpad)
                and frames.untyped_storage().nbytes() // frames.element_size() - frames.storage_offset() >= n * h * w * cpad):
            x = frames.as_strided((n, h, w, cpad), (h * w * cpad, w * cpad, cpad, 1), frames.storage_offset())
        else:
            x = torch.zeros((n, h, w, cpad), dtype=frames.dtype, device=frames.device)
            x[..., :3] = frames.permute(0, 2, 3, 1)
    else:
        raise ValueError(f"{who}: a model input must be [{n},3,{h},{w}] or the padded [{n},{h},{w},{cpad}] buffer, got "
                         f"{tuple(frames.shape)}")
    if x.data_ptr() % 16:
        x = x.clone()
    return x


def _render(who, labels, frames=None, truth=None, ignore_index=None, alphas=(0, 0, 0, 0), palette=None, classes=None,
            void_color=VOID_COLOR, outline=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, counts=None, agreement=None, out=None):
    """The one path to the kernel.  -> (picture, counts, agreement); counts / agreement are what was handed in (None if nothing was)."""
    lab, single = A.label_maps(who, labels)
    n, h, w = lab.shape
    dev = lab.device
    if truth is not None:
        tru, _ = A.label_maps(who, truth, "truth")
        if tuple(tru.shape) != (n, h, w):
            raise ValueError(f"{who}: truth must have the labels' shape {(n, h, w)}, got {tuple(tru.shape)}")
        if tru.dtype != lab.dtype:                                 # one dtype for both: the uint8 one is widened (lossless)
            lab, tru = lab.long(), tru.long()
    else:
        tru = None
    A.int_in(who, "ignore_index", ignore_index, -2 ** 31, 2 ** 31 - 1, True)
    table, classes = _table_for(palette, classes, void_color, dev)
    base = None if frames is None else _base(who, frames, n, h, w, single)
    denorm = _denorm_cached(tuple(mean), tuple(std)) if base is not None and base.dtype != torch.uint8 else None
    line = -1
    if outline is not None:
        r, g, b = _color("outline", OUTLINE_WHITE if outline is True else outline)
        line = r | (g << 8) | (b << 16)
    A.counts_tensor(who, "counts", counts, (n, 256), dev)
    if agreement is not None and tru is None:
        raise ValueError(f"{who}: agreement needs truth")
    A.counts_tensor(who, "agreement", agreement, (n, 3), dev)
    out = A.out_tensor(who, "out", out, (n, h, w, 3), torch.uint8, dev)
    A.on_device(dev, K.render_u8, lab, tru, base, table, n, h, w, classes, ignore_index, alphas, denorm, line, out, counts, agreement)
    return (out[0] if single else out), counts, agreement


def _new_counts(labels, want):
    if not want:
        return None
    n = 1 if labels.dim() == 2 else int(labels.shape[0])
    return torch.zeros((n, 256), dtype=torch.int64, device=labels.device)


def colorize(labels, palette=None, classes=None, outline=None, return_counts=False, void_color=VOID_COLOR, counts=None, out=None):
    """Colour mask of a label map: uint8 ``[N,H,W,3]`` (``[H,W,3]`` for ``[H,W]`` labels) -- the reference's
    ``create_colored_mask`` and the ``true_colored`` / ``pred_colored`` loops of ``train_model``.

    ``palette``: None (``default_palette()``), ``[K,3]`` colours (``load_palette``'s second value), or a ``palette_table``;
    ``classes``: labels at or above it are void and get ``void_color`` (None: the palette's length); ``outline``: None, an RGB
    colour or True (white); ``return_counts``: also the int64 ``[N,256]`` label histogram.  ``counts``: a tensor of the caller's
    to accumulate into (then returned)."""
    if not torch.is_tensor(labels):
        raise ValueError(f"colorize: labels must be a tensor, got {type(labels).__name__}")
    cnt = counts if counts is not None else _new_counts(labels, return_counts)
    pic, cnt, _ = _render("colorize", labels, palette=palette, classes=classes, void_color=void_color, outline=outline, counts=cnt,
                          out=out)
    return (pic, cnt) if (return_counts or counts is not None) else pic


def overlay(frames, labels, palette=None, alpha=0.5, void_alpha=0.0, outline=None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
            return_counts=False, classes=None, void_color=VOID_COLOR, counts=None, out=None):
    """The class colours blended over the frame at opacity ``alpha`` (void labels at ``void_alpha``): uint8 ``[N,H,W,3]`` -- what
    ``viz_utils.create_overlay`` / ``predict.create_overlay`` are for.  ``frames``: uint8 ``[N,H,W,3]``, or the model input
    (``data.prepare_batch``'s view, or its padded NHWC buffer), de-normalised with ``mean`` / ``std``."""
    if not torch.is_tensor(labels):
        raise ValueError(f"overlay: labels must be a tensor, got {type(labels).__name__}")
    a, av = alpha_level(alpha), alpha_level(void_alpha)
    cnt = counts if counts is not None else _new_counts(labels, return_counts)
    pic, cnt, _ = _render("overlay", labels, frames=frames, alphas=(a, av, a, a), palette=palette, classes=classes,
                          void_color=void_color, outline=outline, mean=mean, std=std, counts=cnt, out=out)
    return (pic, cnt) if (return_counts or counts is not None) else pic


def error_map(frames, pred, truth, ignore_index=None, alpha_wrong=1.0, alpha_right=0.0, alpha_void=0.0, palette=None, classes=None,
              outline=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, void_color=VOID_COLOR, agreement=None, out=None):
    """``(picture, agreement)``: the frame with the PREDICTED class colour at opacity ``alpha_wrong`` where the prediction differs
    from a valid truth label, ``alpha_right`` where it agrees and ``alpha_void`` where the truth is void (``== ignore_index`` or
    ``>= classes``); ``agreement``: int64 ``[N,3]`` agree / differ / truth-void pixel counts (accumulating into a tensor of the
    caller's when one is given).  ``frames`` may be None: the colours alone."""
    if not torch.is_tensor(pred):
        raise ValueError(f"error_map: pred must be a tensor, got {type(pred).__name__}")
    if agreement is None:
        agreement = torch.zeros((1 if pred.dim() == 2 else int(pred.shape[0]), 3), dtype=torch.int64, device=pred.device)
    aw, ar, avd = alpha_level(alpha_wrong), alpha_level(alpha_right), alpha_level(alpha_void)
    pic, _, agr = _render("error_map", pred, frames=frames, truth=truth, ignore_index=ignore_index, alphas=(aw, aw, ar, avd),
                          palette=palette, classes=classes, void_color=void_color, outline=outline, mean=mean, std=std,
                          agreement=agreement, out=out)
    return pic, agr


def render_large(model, frame_u8_hwc, tile=512, overlap=0.25, tta=None, palette=None, alpha=0.5, outline=None, classes=None,
                 **predict_large_kwargs):
    """``(labels int64 [H,W], overlay uint8 [H,W,3], counts int64 [256])`` of one frame of any size, all on the device:
    ``predict.predict_large`` and then ONE render call over its labels and the frame."""
    from .predict import MAX_CLASSES, predict_large
    if isinstance(frame_u8_hwc, np.ndarray):
        frame_u8_hwc = torch.from_numpy(np.ascontiguousarray(frame_u8_hwc))
    if not torch.is_tensor(frame_u8_hwc):
        raise ValueError(f"render_large: the frame must be a uint8 [H,W,3] array or tensor, got {type(frame_u8_hwc).__name__}")
    frame = frame_u8_hwc.to(A.model_device(model, "render_large", MAX_CLASSES), non_blocking=True)      # the ONE copy of the frame
    labels = predict_large(model, frame, tile=tile, overlap=overlap, tta=tta, **predict_large_kwargs)
    if classes is None:
        classes = int(model.classes)
    pic, counts = overlay(frame, labels, palette=palette, alpha=alpha, outline=outline, classes=classes, return_counts=True)
    return labels, pic, counts[0]
