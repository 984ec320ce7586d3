"""Numpy mirror of the rendering rule of ``udaseg_render_u8`` (include/udaseg.h, render.py): integer arithmetic with int64
intermediates, fp32 only where the rule says fp32.  The GPU tests compare with ``torch.equal``: there is no tolerance."""
import numpy as np


def labels_ref(labels):
    """-> int64 [N,H,W] in 0..255: an int64 label outside [0, 255] reads as 255."""
    lab = np.asarray(labels)
    if lab.dtype == np.uint8:
        return lab.astype(np.int64)
    assert lab.dtype == np.int64, lab.dtype
    return np.where((lab < 0) | (lab > 255), 255, lab).astype(np.int64)


def table_ref(colours, classes, void_color=(0, 0, 0)):
    """uint8 [256,3]: the palette's colours for 0 .. classes-1, void_color for every other entry."""
    t = np.empty((256, 3), dtype=np.uint8)
    t[:] = np.asarray(void_color, dtype=np.uint8)
    t[:classes] = np.asarray(colours, dtype=np.uint8)[:classes]
    return t


def alpha_ref(alpha):
    """round_half_even(alpha * 256) as an int in [0, 256]."""
    a = int(np.rint(np.float64(alpha) * 256.0))
    assert 0 <= a <= 256, alpha
    return a


def denorm_ref(x, scale, shift):
    """The de-normalisation of a model input: clip(round_half_even(x * scale + shift), 0, 255) per channel, one fp32 multiply and
    one fp32 add (each rounded), NaN -> 0.  x: float32 [..., >=3] (bf16 values widened exactly); scale, shift: 3 floats, taken
    as fp32.  -> int64 [..., 3]."""
    x = np.asarray(x, dtype=np.float32)[..., :3]
    s = np.asarray(scale, dtype=np.float32)
    m = np.asarray(shift, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x * s).astype(np.float32)
        v = (v + m).astype(np.float32)
        v = np.rint(v)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, 0, 255).astype(np.int64)


def blend_ref(b, c, a):
    """(b * (256 - a) + c * a + 128) >> 8 in int64."""
    b, c, a = np.asarray(b, dtype=np.int64), np.asarray(c, dtype=np.int64), np.asarray(a, dtype=np.int64)
    return (b * (256 - a) + c * a + 128) >> 8


def outline_ref(lab):
    """bool [N,H,W]: the label differs from its left, right, upper or lower neighbour inside the same image."""
    e = np.zeros(lab.shape, dtype=bool)
    d = lab[:, :, 1:] != lab[:, :, :-1]
    e[:, :, 1:] |= d
    e[:, :, :-1] |= d
    d = lab[:, 1:, :] != lab[:, :-1, :]
    e[:, 1:, :] |= d
    e[:, :-1, :] |= d
    return e


def category_ref(labels, classes, truth=None, ignore_index=None):
    """int64 [N,H,W] category: 3 truth void, else 2 truth == L, else 1 L void, else 0."""
    lab = labels_ref(labels)
    k = (lab >= classes).astype(np.int64)
    if truth is not None:
        raw = np.asarray(truth).astype(np.int64)
        t = labels_ref(truth)
        tvoid = t >= classes
        if ignore_index is not None:
            tvoid |= raw == int(ignore_index)
        k = np.where(tvoid, 3, np.where(t == lab, 2, k))
    return k


def render_ref(labels, table, classes, base=None, truth=None, ignore_index=None, alpha=(0, 0, 0, 0), outline=None, scale=None,
               shift=None):
    """labels [N,H,W] uint8 / int64; table uint8 [256,3]; base None, uint8 [N,H,W,3] or float32 [N,H,W,>=3] (a model input, with
    scale / shift); truth None or like labels; alpha: four ints in [0, 256]; outline None or an (r, g, b).
    -> (out uint8 [N,H,W,3], counts int64 [N,256], agreement int64 [N,3] or None)."""
    lab = labels_ref(labels)
    n = lab.shape[0]
    c = np.asarray(table, dtype=np.uint8).astype(np.int64)[lab]
    k = category_ref(labels, classes, truth, ignore_index)
    if base is None:
        out = c
    else:
        base = np.asarray(base)
        b = base.astype(np.int64) if base.dtype == np.uint8 else denorm_ref(base, scale, shift)
        a = np.asarray(alpha, dtype=np.int64)[k][..., None]
        out = blend_ref(b, c, a)
    if outline is not None:
        out = np.where(outline_ref(lab)[..., None], np.asarray(outline, dtype=np.int64), out)
    assert out.min() >= 0 and out.max() <= 255
    counts = np.stack([np.bincount(lab[i].ravel(), minlength=256) for i in range(n)]).astype(np.int64)
    agreement = None
    if truth is not None:
        agreement = np.stack([[(k[i] == 2).sum(), ((k[i] == 0) | (k[i] == 1)).sum(), (k[i] == 3).sum()] for i in range(n)]).astype(np.int64)
    return out.astype(np.uint8), counts, agreement
