"""numpy restatement of the frame-ingest definitions (include/udaseg.h, INTEGRATION.md "Frame ingest"): the exact area filter
in int64, nearest indices, the antialiased bilinear tables and their application in float64 (or float32), and the
class-balance formulas via ``np.bincount``.  Written from the definitions; shares no code with ``ingest.py``."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)

# the axis pairs (source, destination) and shapes the definitions were checked on
AXIS_PAIRS = [(96, 32), (100, 32), (150, 64), (37, 32), (33, 32), (4100, 8), (4000, 256), (6000, 256)]
AA_SHAPES = [((100, 150), (32, 64)), ((96, 144), (32, 48)), ((37, 53), (32, 32)), ((64, 64), (64, 64)), ((48, 40), (64, 96)),
             ((300, 500), (256, 256))]


# ------------------------------------------------------------------------------------------------------------------ area
def box_weights(L, l):
    """Dense int64 ``[l, L]``: the overlap of destination cell ``[i*L, (i+1)*L)`` with source cell ``[s*l, (s+1)*l)``."""
    i = np.arange(l, dtype=np.int64)[:, None]
    s = np.arange(L, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * L, (s + 1) * l) - np.maximum(i * L, s * l))


def _fold_axis(a, l):
    """Sums axis 1 of ``a`` ``[n, L, ...]`` with the box weights of ``L -> l``, one destination index at a time: the whole source
    cells in one unweighted int64 sum (times ``l``), the at most two cells cut by the destination cell's ends on their own."""
    L = a.shape[1]
    out = np.zeros((a.shape[0], l) + a.shape[2:], dtype=np.int64)
    for i in range(l):
        lo, hi = i * L, (i + 1) * L
        s0, s1 = lo // l, -(-hi // l)
        first = min(hi, (s0 + 1) * l) - lo                    # weight of cell s0
        last = hi - max(lo, (s1 - 1) * l)                     # weight of cell s1 - 1
        f0 = s0 if first == l else s0 + 1
        f1 = s1 if last == l else s1 - 1
        if f1 > f0:
            out[:, i] += l * a[:, f0:f1].sum(axis=1, dtype=np.int64)
        if first != l:
            out[:, i] += first * a[:, s0].astype(np.int64)
        if last != l and s1 - 1 > s0:
            out[:, i] += last * a[:, s1 - 1].astype(np.int64)
    return out


def area_total(src, h, w):
    """int64 ``[n, h, w, 3]``: ``sum_s sum_t wy(i,s) * wx(j,t) * src[s][t]`` of uint8 ``src`` ``[n, H, W, 3]``."""
    v = _fold_axis(src, h)                                    # [n, h, W, 3]
    return _fold_axis(v.transpose(0, 2, 1, 3), w).transpose(0, 2, 1, 3)


def area_resize(src, h, w):
    """uint8 ``[n, h, w, 3]``: ``floor((2*total + H*W) / (2*H*W))``."""
    n, H, W, _ = src.shape
    hw = np.int64(H) * np.int64(W)
    return ((2 * area_total(src, h, w) + hw) // (2 * hw)).astype(np.uint8)


def area_resize_dense(src, h, w):
    """The same by the dense weight matrices (small shapes only)."""
    n, H, W, _ = src.shape
    total = np.einsum("is,jt,nstc->nijc", box_weights(H, h), box_weights(W, w), src.astype(np.int64))
    hw = np.int64(H) * np.int64(W)
    return ((2 * total + hw) // (2 * hw)).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------- nearest
def nearest_index(L, l):
    return (np.arange(l, dtype=np.int64) * L) // l


def nearest_resize(src, h, w):
    """``[n, H, W]`` -> ``[n, h, w]``: ``src[(i*H)//h][(j*W)//w]``."""
    return src[:, nearest_index(src.shape[1], h)][:, :, nearest_index(src.shape[2], w)]


# ------------------------------------------------------------------------------------------------- antialiased bilinear
def aa_matrix(L, l):
    """Dense float64 ``[l, L]`` of ``interpolate(mode="bilinear", antialias=True, align_corners=False)`` along one axis."""
    m = np.zeros((l, L), dtype=np.float64)
    scale = L / l
    support = max(scale, 1.0)
    for i in range(l):
        c = scale * (i + 0.5)
        lo, hi = max(0, int(c - support + 0.5)), min(L, int(c + support + 0.5))
        wt = np.array([max(0.0, 1.0 - abs((j - c + 0.5) / support)) for j in range(lo, hi)], dtype=np.float64)
        m[i, lo:hi] = wt / wt.sum()
    return m


def normalize(v, dt):
    """A.Normalize with ``data.prepare_batch``'s arithmetic: (v - mean255) * inv_std255, both constants rounded to fp32 first."""
    mean = (MEAN * np.float32(255.0)).astype(dt)
    inv = np.reciprocal(STD * np.float32(255.0), dtype=np.float32).astype(dt)
    return (v - mean) * inv


def aa_resize(src, h, w):
    """float64 ``[n, h, w, 3]`` on the 0..255 scale."""
    n, H, W, _ = src.shape
    return np.einsum("is,jt,nstc->nijc", aa_matrix(H, h), aa_matrix(W, w), src.astype(np.float64), optimize=True)


# --------------------------------------------------------------------------------------------------------- class balance
def mask_hist(masks):
    """int64 ``[n, 256]``."""
    return np.stack([np.bincount(m.reshape(-1), minlength=256) for m in masks]).astype(np.int64)


def class_stats(masks):
    stats = mask_hist(masks).sum(axis=0)
    return {int(v): int(stats[v]) for v in np.nonzero(stats)[0]}


def sample_weights(masks):
    """Per mask ``sum_c (count_c / size) * (total / stats_c)``, normalised to sum 1."""
    hist = mask_hist(masks)
    stats = hist.sum(axis=0)
    total = float(stats.sum())
    out = np.zeros(len(masks), dtype=np.float64)
    for k, row in enumerate(hist):
        size = float(row.sum())
        for c in np.nonzero(row)[0]:
            out[k] += (row[c] / size) * (total / float(stats[c]))
    return out / out.sum()
