"""numpy mirror of the class-mixing contract (``mix.py``'s module docstring): the selection through ``_strong_aug_ref``'s
Philox4x32-10, the mixing and its counts.  Integers only: the device results must equal these bit for bit."""
import numpy as np

from _strong_aug_ref import philox4x32_10


def keys_u32(keys):
    """``[n, 2]`` keys as drawn (int64 in ``[0, 2^32)``) or as int32 bit patterns -> uint32."""
    return (np.asarray(keys).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def mask_hist(masks):
    """uint8 ``[n, ...]`` -> int64 ``[n, 256]``."""
    m = np.asarray(masks)
    return np.stack([np.bincount(m[i].reshape(-1), minlength=256) for i in range(m.shape[0])]).astype(np.int64)


def select(hist, classes, keys, min_pixels=1):
    """int32 ``[n]``: half of the present classes of every row (rounded up) by a partial Fisher-Yates on Philox words."""
    hist, keys = np.asarray(hist), keys_u32(keys)
    sel = np.zeros(hist.shape[0], dtype=np.uint32)
    for i in range(hist.shape[0]):
        present = [c for c in range(classes) if hist[i, c] >= min_pixels]
        P = len(present)
        bits = 0
        for j in range((P + 1) // 2):
            r = int(philox4x32_10(np.array([j, 0, 0, 0], dtype=np.uint32), keys[i])[0])
            t = j + ((r * (P - j)) >> 32)
            present[j], present[t] = present[t], present[j]
            bits |= 1 << present[j]
        sel[i] = bits
    return sel.view(np.int32)


def mix(src, src_masks, tgt, tgt_masks, sel, boxes, classes, void=255):
    """-> (frames uint8 [n,h,w,3], masks uint8 [n,h,w], counts int64 [n,3]) of ONE call."""
    src, src_masks, tgt = np.asarray(src), np.asarray(src_masks), np.asarray(tgt)
    n, h, w = src_masks.shape
    bits = np.asarray(sel).astype(np.int64) & 0xFFFFFFFF
    s = src_masks.astype(np.int64)
    m = (s < classes) & (((bits[:, None, None] >> np.minimum(s, 31)) & 1) == 1)
    if boxes is not None:
        b = np.asarray(boxes).astype(np.int64)
        y, x = np.arange(h)[None, :, None], np.arange(w)[None, None, :]
        m = m | ((y >= b[:, 0, None, None]) & (y < b[:, 2, None, None]) & (x >= b[:, 1, None, None]) & (x < b[:, 3, None, None]))
    other = np.full((n, h, w), void, dtype=np.uint8) if tgt_masks is None else np.asarray(tgt_masks)
    frames = np.where(m[..., None], src, tgt).astype(np.uint8)
    masks = np.where(m, src_masks, other).astype(np.uint8)
    counts = np.stack([m.sum(axis=(1, 2)), (~m & (other < classes)).sum(axis=(1, 2)), (~m & (other >= classes)).sum(axis=(1, 2))],
                      axis=1).astype(np.int64)
    return frames, masks, counts
