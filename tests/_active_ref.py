"""Numpy mirror of the window votes and the acquisition scores (active.py, csrc/window.hip), written from the definitions of
include/udaseg.h: the per-class window counts by integral images (NOT the packed two-pass form the kernel uses), every float product
in plain float64, and beside it an fp32 evaluation of the same product in the operation order the header states -- the grade files'
bar is 4 x the deviation of that fp32 leg from the float64 one.  Also the map and score generators the host and GPU tests share."""
import numpy as np

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------- labels, counts
def read(labels):
    """int64 [n,h,w] of a uint8 or int64 label map: an int64 value outside [0, 255] reads as 255."""
    a = np.asarray(labels)
    if a.ndim == 2:
        a = a[None]
    a = a.astype(np.int64)
    return np.where((a < 0) | (a > 255), 255, a)


def void_of(L, classes, ignore_index):
    v = L >= classes
    return v if ignore_index is None else v | (L == ignore_index)


def box(a, r):
    """Sum of ``a`` [..., h, w] over the (2r+1)^2 window clipped at the frame, by an integral image (exact for integers)."""
    h, w = a.shape[-2:]
    ii = np.zeros(a.shape[:-2] + (h + 1, w + 1), dtype=a.dtype)
    ii[..., 1:, 1:] = a.cumsum(-2).cumsum(-1)
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r + 1, h)
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r + 1, w)
    return (ii[..., y1[:, None], x1[None, :]] - ii[..., y0[:, None], x1[None, :]] - ii[..., y1[:, None], x0[None, :]]
            + ii[..., y0[:, None], x0[None, :]])


def counts(labels, r, classes, ignore_index=None):
    """(n_c int64 [n,classes,h,w], L int64 [n,h,w], void bool [n,h,w])."""
    L = read(labels)
    v = void_of(L, classes, ignore_index)
    onehot = ((L[:, None] == np.arange(classes)[None, :, None, None]) & ~v[:, None]).astype(np.int64)
    return box(onehot, r), L, v


def counts_brute(labels, r, classes, ignore_index=None):
    """The same by plain loops over the window (tiny maps only)."""
    L = read(labels)
    v = void_of(L, classes, ignore_index)
    n, h, w = L.shape
    out = np.zeros((n, classes, h, w), dtype=np.int64)
    for i in range(n):
        for y in range(h):
            for x in range(w):
                for yy in range(max(0, y - r), min(h, y + r + 1)):
                    for xx in range(max(0, x - r), min(w, x + r + 1)):
                        if not v[i, yy, xx]:
                            out[i, L[i, yy, xx], y, x] += 1
    return out


def mode(labels, r, classes, ignore_index, fill_void, void_label):
    """(out uint8 [n,h,w], agreement fp32 [n,h,w], counts int64 [n,3]: changed, void filled, void left)."""
    nc, L, v = counts(labels, r, classes, ignore_index)
    n = nc.sum(1)
    best = nc.max(1)
    m = nc.argmax(1)                                                           # the smallest class among the tied
    own = np.take_along_axis(nc, np.where(v, 0, L)[:, None], axis=1)[:, 0]
    m = np.where(~v & (own == best), L, m)                                     # the centre's own label if it is among them
    out = np.where(v, np.where(fill_void & (n > 0), m, void_label), m).astype(np.uint8)
    with np.errstate(invalid="ignore", divide="ignore"):
        agr = np.where(n > 0, best.astype(F32) / n.astype(F32), F32(0)).astype(F32)
    flat = lambda a: a.reshape(len(L), -1).sum(1)
    cnt = np.stack([flat(~v & (m != L)), flat(v & bool(fill_void) & (n > 0)), flat(v & ~(bool(fill_void) & (n > 0)))], axis=1)
    return out, agr, cnt.astype(np.int64)


def table(r):
    m = np.arange((2 * r + 1) ** 2 + 1, dtype=F64)
    return (m * np.log(np.maximum(m, 1.0))).astype(F32)


def impurity_of_counts(nc, classes, r):
    """(float64, fp32) [n,h,w] of the counts: the definition in float64; the header's fp32 evaluation."""
    n = nc.sum(1)
    ncf = nc.astype(F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s64 = (ncf * np.log(np.maximum(ncf, 1.0))).sum(1)
        i64 = np.where(n > 1, (np.log(np.maximum(n, 1)) - s64 / np.maximum(n, 1)) / np.log(F64(classes)), 0.0)
    T = table(r)
    S = np.zeros(n.shape, dtype=F32)
    for c in range(classes):                                                   # ascending class order
        S = (S + T[nc[:, c]]).astype(F32)
    den = (n.astype(F32) * F32(np.log(F64(classes)))).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        i32 = np.where(n > 1, np.clip(((T[n] - S).astype(F32) / den).astype(F32), F32(0), F32(1)), F32(0)).astype(F32)
    return np.clip(i64, 0.0, 1.0), i32


def impurity(labels, r, classes, ignore_index=None):
    nc, _, _ = counts(labels, r, classes, ignore_index)
    return impurity_of_counts(nc, classes, r)


# ------------------------------------------------------------------------------------------------------------------- scores
def prepare(scores, classes, probs=False):
    """scores fp32 [n,C,h,w] -> (labels uint8, entropy float64, entropy fp32, counters int64 [2]) per udaseg_acquire_prepare."""
    z = np.asarray(scores, dtype=F32)[:, :classes]
    fin = np.isfinite(z).all(1)
    zz = np.where(fin[:, None], z, F32(0))
    lab = np.where(fin, zz.argmax(1), 255).astype(np.uint8)
    s64, s32 = 1.0 / np.log(F64(classes)), F32(1) / np.log(F32(classes))
    with np.errstate(invalid="ignore", divide="ignore"):
        if probs:
            p64 = zz.astype(F64)
            lp64 = np.log(p64)
            p32, lp32 = zz, np.log(zz)
        else:
            d64 = zz.astype(F64) - zz.astype(F64).max(1, keepdims=True)
            lp64 = d64 - np.log(np.exp(d64).sum(1, keepdims=True))
            p64 = np.exp(lp64)
            d32 = (zz - zz.max(1, keepdims=True)).astype(F32)
            sm = np.zeros(fin.shape, dtype=F32)
            for c in range(classes):
                sm = (sm + np.exp(d32[:, c]).astype(F32)).astype(F32)
            lp32 = (d32 - np.log(sm).astype(F32)[:, None]).astype(F32)
            p32 = np.exp(lp32).astype(F32)
        h64 = np.where(p64 > 0, -(s64 * (p64 * lp64)), 0.0).sum(1)
        h32 = np.zeros(fin.shape, dtype=F32)
        for c in range(classes):
            term = np.where(p32[:, c] > 0, -(s32 * (p32[:, c] * lp32[:, c]).astype(F32)).astype(F32), F32(0))
            h32 = (h32 + term).astype(F32)
    fin = fin & np.isfinite(h32)
    lab = np.where(fin, lab, 255).astype(np.uint8)
    return lab, np.where(fin, h64, 0.0), np.where(fin, h32, F32(0)).astype(F32), np.array([fin.sum(), (~fin).sum()], dtype=np.int64)


def window_sum32(e, r):
    """fp32 box sum in the header's order: per row 2r+1 terms left to right, then 2r+1 row sums top to bottom (0 outside)."""
    n, h, w = e.shape
    pad = np.zeros((n, h + 2 * r, w + 2 * r), dtype=F32)
    pad[:, r:r + h, r:r + w] = e
    rows = pad[:, :, 0:w].copy()
    for j in range(1, 2 * r + 1):
        rows = (rows + pad[:, :, j:j + w]).astype(F32)
    out = rows[:, 0:h].copy()
    for j in range(1, 2 * r + 1):
        out = (out + rows[:, j:j + h]).astype(F32)
    return out


def score(labels_u8, entropy32, r, classes, kind, exclude=None):
    """The score and key of uint8 labels and an fp32 entropy map, as (score64, key64, score32, key32, candidate bool)."""
    nc, L, v = counts(labels_u8, r, classes, None)
    n = nc.sum(1)
    i64, i32 = impurity_of_counts(nc, classes, r)
    e = np.where(v, F32(0), np.asarray(entropy32, dtype=F32))
    with np.errstate(invalid="ignore", divide="ignore"):
        u64 = np.where(n > 0, box(e.astype(F64), r) / np.maximum(n, 1), 0.0)
        u32 = np.where(n > 0, (window_sum32(e, r) / np.maximum(n, 1).astype(F32)).astype(F32), F32(0)).astype(F32)
    a64 = (i64 * u64, i64, u64)[kind]
    a32 = ((i32 * u32).astype(F32), i32, u32)[kind]
    cand = ~v & (a32 > 0) & np.isfinite(a32)
    a64, a32 = np.minimum(a64, 1.0), np.minimum(a32, F32(1))                   # A = min(A0, 1): the key never falls below 0
    if exclude is not None:
        cand &= np.asarray(exclude) == 0
    return (np.where(cand, a64, 0.0), np.where(cand, 1.0 - a64, -1.0), np.where(cand, a32, F32(0)).astype(F32),
            np.where(cand, F32(1) - a32, F32(-1)).astype(F32), cand)


def cells(key32, ch, cw):
    """(cell_key float64, cell_key fp32 with a sequential fp32 sum, has-candidate bool) [n, gh, gw] of an fp32 key map."""
    n, h, w = key32.shape
    gh, gw = -(-h // ch), -(-w // cw)
    k64, k32, has = np.full((n, gh, gw), -1.0), np.full((n, gh, gw), F32(-1)), np.zeros((n, gh, gw), dtype=bool)
    for i in range(n):
        for cy in range(gh):
            for cx in range(gw):
                blk = key32[i, cy * ch:(cy + 1) * ch, cx * cw:(cx + 1) * cw]
                a = (F32(1) - blk[blk >= 0]).astype(F32)
                if a.size:
                    has[i, cy, cx] = True
                    k64[i, cy, cx] = 1.0 - (1.0 - blk[blk >= 0].astype(F64)).sum() / blk.size
                    k32[i, cy, cx] = F32(1) - F32(np.cumsum(a, dtype=F32)[-1] / F32(blk.size))
    return k64, k32, has


def select(key, k, into=None):
    """The mask of the k smallest keys >= 0 of every image with every tie of the last one, OR-ed into ``into``; (mask uint8,
    counts int64 [n,2]: newly selected, candidates; the size of the tie group at the threshold per image)."""
    key = np.asarray(key)
    n = key.shape[0]
    mask = np.zeros(key.shape, dtype=np.uint8) if into is None else np.array(into, dtype=np.uint8)
    cnt, ties = np.zeros((n, 2), dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in range(n):
        cand = key[i] >= 0
        vals = np.sort(key[i][cand])                                          # 1. sort the candidates
        if vals.size == 0:
            continue
        thr = vals[min(k, vals.size) - 1]                                      # 2. the threshold at rank k
        sel = cand & (key[i] <= thr)                                           # 3. every tie
        ties[i] = int((vals == thr).sum())
        cnt[i] = [int((sel & (mask[i] == 0)).sum()), int(cand.sum())]
        mask[i] |= sel.astype(np.uint8)
    return mask, cnt, ties


def expand(cell_mask, h, w, ch, cw, into=None):
    big = np.repeat(np.repeat(np.asarray(cell_mask), ch, axis=1), cw, axis=2)[:, :h, :w]
    return (big != 0).astype(np.uint8) | (0 if into is None else np.asarray(into))


# --------------------------------------------------------------------------------------------------------------- generators
VOID = 255
SHAPES = [(1, 1, 1, 1), (2, 1, 7, 3), (2, 7, 1, 3), (3, 5, 9, 16), (2, 33, 65, 0), (2, 33, 65, 1), (2, 70, 131, 5), (1, 97, 150, 13),
          (65, 9, 13, 2)]
CLASS_COUNTS = (2, 23, 32)
CASES = [(n, h, w, r, c) for (n, h, w, r) in SHAPES for c in CLASS_COUNTS]


def roomy(h, w, r):
    """The map holds whole blocks of make_map: a clean centre, a texture and a void block all fit."""
    return r >= 1 and h >= 2 * (2 * r + 3) and w >= 3 * (2 * r + 3)


def make_map(n, h, w, r, classes, seed=0):
    """uint8 [n,h,w]: constant blocks of side 2r + 3 whose neighbours differ in class (the centre's window is pure), every third
    block filled with per-pixel texture of the labels 0 .. classes + 1 (two of them beyond the classes: void), a void speck (255)
    in every third block, and one whole block of void per image (its centre has an empty window)."""
    rng = np.random.RandomState(1000 * seed + 131 * n + 17 * h + 3 * w + r + 7 * classes)
    S = 2 * r + 3
    by, bx = np.arange(h) // S, np.arange(w) // S
    m = np.empty((n, h, w), dtype=np.uint8)
    for i in range(n):
        kind = (by[:, None] + bx[None, :] + i) % 3
        base = ((by[:, None] + 2 * bx[None, :] + i) % classes).astype(np.uint8)
        tex = rng.randint(0, classes + 2, size=(h, w)).astype(np.uint8)
        img = np.where(kind == 1, tex, base)
        speck = (kind == 2) & (np.arange(h)[:, None] % S == 1) & (np.arange(w)[None, :] % S == 1)
        img[speck] = VOID
        img[(by[:, None] == 1) & (bx[None, :] == (i % 2))] = VOID
        m[i] = img
    return m


def as_int64(m, seed=0):
    """The int64 form of a uint8 map with half of its 255s replaced by values outside [0, 255] (which read as 255)."""
    a = m.astype(np.int64)
    idx = np.flatnonzero(a == 255)
    rng = np.random.RandomState(seed + 5)
    pick = idx[rng.rand(idx.size) < 0.5]
    a.reshape(-1)[pick] = np.where(rng.rand(pick.size) < 0.5, -1, 1000)
    return a


GAP = 1e-3


def make_scores(n, h, w, r, classes, seed=0, probs=False):
    """fp32 [n,classes,h,w] logits (or probabilities) that follow make_map's regions with noise, the top-two gap of every finite
    row at least GAP (2 x GAP before the softmax of the probs form), and a sprinkle of rows with a NaN or an infinity."""
    rng = np.random.RandomState(77 + 1000 * seed + 131 * n + 17 * h + 3 * w + r + 7 * classes)
    m = make_map(n, h, w, r, classes, seed + 1).astype(np.int64)
    z = rng.randn(n, classes, h, w) * 1.5
    onehot = m[:, None] == np.arange(classes)[None, :, None, None]
    z = z + 3.0 * onehot * rng.rand(n, 1, h, w)
    if probs:
        z = np.exp(z - z.max(1, keepdims=True))
        z = z / z.sum(1, keepdims=True)
    z = z.astype(F32)
    srt = np.sort(z, axis=1)
    close = (srt[:, -1] - srt[:, -2]) < (GAP if probs else 2 * GAP)
    top = z.argmax(1)
    bump = np.zeros_like(z)
    np.put_along_axis(bump, top[:, None], (close * (4 * GAP)).astype(F32)[:, None], axis=1)
    z = (z + bump).astype(F32)
    bad = rng.rand(n, h, w) < 0.01
    ch = rng.randint(0, classes, size=(n, h, w))
    val = np.where(rng.rand(n, h, w) < 0.5, np.nan, np.inf).astype(F32)
    cur = np.take_along_axis(z, ch[:, None], axis=1)[:, 0]
    np.put_along_axis(z, ch[:, None], np.where(bad, val, cur)[:, None], axis=1)
    return z


def top_two_gap(z, classes):
    z = np.asarray(z)[:, :classes]
    fin = np.isfinite(z).all(1)
    srt = np.sort(np.where(fin[:, None], z, 0), axis=1)
    return np.where(fin, srt[:, -1] - srt[:, -2], np.inf)


# the selection cases of the GPU test: (n, h, w, radius, classes, kind, budget, cell)
SELECT_CASES = [(2, 33, 65, 1, 5, 0, 40, None), (2, 33, 65, 1, 5, 1, 0.05, None), (3, 30, 45, 2, 23, 0, 0.02, None),
                (2, 33, 65, 1, 5, 0, 6, (8, 8)), (2, 33, 65, 2, 23, 2, 0.25, (8, 8))]
