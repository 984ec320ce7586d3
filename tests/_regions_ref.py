"""Numpy mirror of the region products (regions.py, csrc/regions.hip), written from the definitions of include/udaseg.h: the pairs
of adjacent pixels are listed by shifted comparisons and joined by a union-find over whole arrays (every root hooks to the smallest
root it touches, then every chain is halved until it is flat; repeated to a fixed point) -- NOT the tiles and merge levels of the
kernels.  Integers only: the GPU tests compare for equality.  tests/test_regions_host.py pins it to scipy.ndimage.label.  Also the
map makers the host and GPU tests share."""
import numpy as np

TILE = (64, 64)               # what udaseg_regions_tile reports (the GPU tests ask the library and pass it in)
CLASSES = 6
VOID = 255
HIST_BINS = 32


def read(labels):
    """int64 [n,h,w] of a uint8 or int64 label map: an int64 value outside [0, 255] reads as 255."""
    a = np.asarray(labels)
    if a.ndim == 2:
        a = a[None]
    a = a.astype(np.int64)
    return np.where((a < 0) | (a > 255), 255, a)


def void_of(L, ignore_index):
    return np.zeros(L.shape, dtype=bool) if ignore_index is None else (L == ignore_index)


def _ids_image(img, void, connectivity):
    h, w = img.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    live = ~void
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    A, B = [], []
    for dy, dx in steps:                                           # pixel (y, x) against (y + dy, x + dx), both inside the image
        ya, yb = slice(0, h - dy), slice(dy, h)
        xa, xb = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
        adj = (img[ya, xa] == img[yb, xb]) & live[ya, xa] & live[yb, xb]
        A.append(idx[ya, xa][adj])
        B.append(idx[yb, xb][adj])
    A, B = np.concatenate(A), np.concatenate(B)
    par = idx.reshape(-1).copy()
    while True:
        ra, rb = par[A], par[B]
        if np.array_equal(ra, rb):
            break
        m = np.minimum(ra, rb)
        np.minimum.at(par, ra, m)
        np.minimum.at(par, rb, m)
        while True:
            pp = par[par]
            if np.array_equal(pp, par):
                break
            par = pp
    out = par.reshape(h, w).astype(np.int32)
    out[void] = -1
    return out


def ids(labels, connectivity=4, ignore_index=None):
    """int32 [n,h,w]: the smallest y * w + x of every pixel's component, -1 on void pixels."""
    assert connectivity in (4, 8)
    L = read(labels)
    V = void_of(L, ignore_index)
    return np.stack([_ids_image(L[i], V[i], connectivity) for i in range(L.shape[0])])


def areas(id_map):
    """int32 [n,h,w] from ``ids``: the number of pixels that share the pixel's id, 0 on void pixels."""
    out = np.zeros(id_map.shape, dtype=np.int32)
    for i in range(id_map.shape[0]):
        flat = id_map[i].reshape(-1)
        ok = flat >= 0
        cnt = np.bincount(flat[ok], minlength=flat.size)
        out[i].reshape(-1)[ok] = cnt[flat[ok]]
    return out


def roots(id_map):
    n, h, w = id_map.shape
    return id_map == np.arange(h * w, dtype=np.int64).reshape(1, h, w)


def min_area_table(min_area):
    t = np.zeros(256, dtype=np.int64)
    if np.ndim(min_area) == 0:
        t[:] = int(min_area)
    else:
        t[: len(min_area)] = np.asarray(min_area, dtype=np.int64)
    return t


def sieve(labels, min_area, connectivity=4, void=255, ignore_index=VOID):
    """(uint8 [n,h,w], int64 [n,3]): the mask with ``void`` on the components below their class's threshold, and per image the
    pixels voided, the components removed and the components kept."""
    L = read(labels)
    I = ids(labels, connectivity, ignore_index)
    Ar = areas(I)
    live = I >= 0
    small = live & (Ar < min_area_table(min_area)[L])
    out = np.where(small, void, L).astype(np.uint8)
    rt = roots(I)
    counts = np.stack([small.sum(axis=(1, 2)), (rt & small).sum(axis=(1, 2)), (rt & ~small).sum(axis=(1, 2))], axis=1)
    return out, counts.astype(np.int64)


def stats(labels, classes, connectivity=4, ignore_index=None):
    """int64 [classes,34]: components, pixels and hist[floor(log2(area))] per class; a label >= classes counts nowhere."""
    L = read(labels)
    I = ids(labels, connectivity, ignore_index)
    Ar = areas(I)
    rt = roots(I)
    out = np.zeros((classes, 2 + HIST_BINS), dtype=np.int64)
    for l, a in zip(L[rt].tolist(), Ar[rt].tolist()):
        if l < classes:
            out[l, 0] += 1
            out[l, 1] += a
            out[l, 2 + a.bit_length() - 1] += 1
    return out


# ------------------------------------------------------------------------------------------------------------------ maps
def as_int64(m, seed=0):
    """The int64 form of a uint8 map with half of its 255s replaced by values outside [0, 255] (which read as 255)."""
    a = m.astype(np.int64)
    idx = np.flatnonzero(a == 255)
    rng = np.random.RandomState(seed + 5)
    pick = idx[rng.rand(idx.size) < 0.5]
    a.reshape(-1)[pick] = np.where(rng.rand(pick.size) < 0.5, -1, 1 << 40)
    return a


def shapes(tile=TILE):
    th, tw = tile
    return [(1, 1, 1), (2, 1, 7), (2, 7, 1), (3, 5, 9), (2, th + 1, tw + 1), (1, 3 * th + 5, 3 * tw + 7), (1, 5 * th + 3, 5 * tw + 1),
            (65, 9, 13)]


def make_map(n, h, w, seed=0):
    """uint8 [n,h,w]: constant blocks of side 5 of the labels 0..2, a twelfth of the pixels relabelled 0..3 one by one, void specks
    (255), a cross of label 4 through the middle row and column (it spans every seam), and -- images must never join -- the last
    row of image i and the first row of image i + 1 both of label 1."""
    rng = np.random.RandomState(1000 * seed + 131 * n + 17 * h + 3 * w)
    coarse = rng.randint(0, 3, size=(n, h // 5 + 1, w // 5 + 1))
    m = np.repeat(np.repeat(coarse, 5, axis=1), 5, axis=2)[:, :h, :w].astype(np.uint8)
    u = rng.rand(n, h, w)
    m[u < 1 / 12] = rng.randint(0, 4, size=int((u < 1 / 12).sum())).astype(np.uint8)
    m[(u > 0.97)] = VOID
    if h >= 3 and w >= 3:
        m[:, h // 2, :] = 4
        m[:, :, w // 2] = 4
    for i in range(n - 1):
        m[i, -1, :] = 1
        m[i + 1, 0, :] = 1
    return m


def split_column(tiles_x, tw):
    """The first column right of the highest-level seam: the U's second arm stands beyond it."""
    k = 1
    while 2 * k < tiles_x:
        k *= 2
    return k * tw


STRUCTURES = ("constant", "checker", "diagonals", "u", "serpentine", "fenced", "random")
TELLS_4_FROM_8 = ("checker", "diagonals", "random")


def structure(name, h, w, tile=TILE):
    """uint8 [1,h,w], each placed on and beside the seams of ``tile`` (h and w: at least three tiles and a few pixels)."""
    th, tw = tile
    m = np.zeros((1, h, w), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if name == "constant":                      # one component of h * w pixels
        m[:] = 3
    elif name == "checker":                     # h * w components of one pixel, or two
        m[0] = 1 + ((y + x) & 1)
    elif name == "diagonals":                   # one-pixel lines through corners of four tiles: \ in label 5, / in label 6
        for cy, cx, anti in ((th, tw, 0), (2 * th, 2 * tw, 0), (th, 2 * tw, 1), (2 * th, tw, 1)):
            for k in range(-7, 7):              # \: (cy - 1, cx - 1) then (cy, cx);  /: (cy, cx - 1) then (cy - 1, cx)
                if anti:
                    m[0, cy - 1 - k, cx + k] = 6
                else:
                    m[0, cy + k, cx + k] = 5
    elif name == "u":                           # the arms meet only in the last tile row; the root is the top of the left arm
        x2 = split_column((w + tw - 1) // tw, tw) + 5
        assert x2 < w - 1 and h - 3 >= ((h - 1) // th) * th
        m[0, 2:h - 2, 5] = 7
        m[0, 2:h - 2, x2] = 7
        m[0, h - 3, 5:x2 + 1] = 7
    elif name == "serpentine":                  # every second row, joined at alternating ends
        m[0, 0::2, :] = 8
        m[0, 1::4, w - 1] = 8
        m[0, 3::4, 0] = 8
    elif name == "fenced":                      # void fences on a seam column and beside a seam row cut label 2 in three
        m[:] = 2
        m[0, :, tw] = VOID
        m[0, th - 1, :tw] = VOID
    elif name == "random":                      # three labels per pixel, the largest near the 8-neighbour percolation threshold
        u = np.random.RandomState(h * 7 + w).rand(h, w)
        m[0] = np.where(u < 0.45, 0, np.where(u < 0.8, 1, 2))
    else:
        raise KeyError(name)
    return m


def seams_spanned(id_map, tile=TILE):
    """The largest number of tile seams the bounding box of one component crosses (columns plus rows), over image 0."""
    th, tw = tile
    h, w = id_map.shape[1:]
    flat = id_map[0].reshape(-1)
    ok = flat >= 0
    ty, tx = (np.arange(h * w) // w) // th, (np.arange(h * w) % w) // tw
    best = 0
    lo_y, hi_y = np.full(h * w, 1 << 30), np.full(h * w, -1)
    lo_x, hi_x = lo_y.copy(), hi_y.copy()
    np.minimum.at(lo_y, flat[ok], ty[ok])
    np.maximum.at(hi_y, flat[ok], ty[ok])
    np.minimum.at(lo_x, flat[ok], tx[ok])
    np.maximum.at(hi_x, flat[ok], tx[ok])
    seen = hi_y >= 0
    if seen.any():
        best = int(((hi_y - lo_y) + (hi_x - lo_x))[seen].max())
    return best
