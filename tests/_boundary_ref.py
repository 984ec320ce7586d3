"""Numpy mirror of the four boundary products (boundary.py, csrc/boundary.hip), written from the definitions of include/udaseg.h:
the boundary flags by shifted comparisons, the distance as the brute-force minimum over the boundary pixels -- every offset of
the disc of radius R is tried against the flag map, NOT the two-pass (column, then row) form the kernel uses.  Integers and a
table lookup only: the GPU tests compare bit for bit.  Also the map generators the host and GPU tests share."""
import numpy as np


def read(labels):
    """int64 [n,h,w] of a uint8 or int64 label map: an int64 value outside [0, 255] reads as 255."""
    a = np.asarray(labels)
    if a.ndim == 2:
        a = a[None]
    a = a.astype(np.int64)
    return np.where((a < 0) | (a > 255), 255, a)


def void_of(L, ignore_index):
    return np.zeros(L.shape, dtype=bool) if ignore_index is None else (L == ignore_index)


def flags(L, void):
    """bool [n,h,w]: a 4-neighbour inside the same image has another label and neither pixel is void."""
    B = np.zeros(L.shape, dtype=bool)
    live = ~void
    for axis in (1, 2):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        d = (L[a] != L[b]) & live[a] & live[b]
        B[a] |= d
        B[b] |= d
    return B


def d2_of_flags(B, R):
    """int32 [n,h,w]: min over the boundary pixels within the disc of (dy^2 + dx^2), R^2 + 1 where there is none."""
    n, h, w = B.shape
    far = R * R + 1
    out = np.full(B.shape, far, dtype=np.int32)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            c = dy * dy + dx * dx
            if c > R * R or abs(dy) >= h or abs(dx) >= w:
                continue
            # pixel (y, x) sees the boundary pixel (y + dy, x + dx)
            ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
            xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
            view = out[:, yd, xd]
            np.minimum(view, np.where(B[:, ys, xs], c, far).astype(np.int32), out=view)
    return out


def d2(labels, R, ignore_index=None):
    L = read(labels)
    return d2_of_flags(flags(L, void_of(L, ignore_index)), R)


def slots(labels, R, ignore_index=None):
    L = read(labels)
    v = void_of(L, ignore_index)
    return np.where(v, R * R + 2, d2_of_flags(flags(L, v), R)).astype(np.int64)


def lookup(labels, R, table, ignore_index=None):
    return np.asarray(table, dtype=np.float32)[slots(labels, R, ignore_index)]


def erode(labels, R, ignore_index, void_label):
    """(uint8 [n,h,w], int64 [n,2]: voided by this call, void already)."""
    L = read(labels)
    v = void_of(L, ignore_index)
    hit = ~v & (d2_of_flags(flags(L, v), R) <= R * R)
    out = np.where(hit, void_label, L).astype(np.uint8)
    counts = np.stack([hit.reshape(len(L), -1).sum(1), v.reshape(len(L), -1).sum(1)], axis=1).astype(np.int64)
    return out, counts


def stats(pred, truth, R, classes, ignore_index=None):
    """(int64 [classes,3]: truth band, predicted band, both; int64 [2]: the trimap's pixels, those predicted right)."""
    T, P = read(truth), read(pred)
    vt = void_of(T, ignore_index)
    vp = void_of(P, ignore_index) | vt
    in_t = ~vt & (d2_of_flags(flags(T, vt), R) <= R * R)
    in_p = ~vp & (d2_of_flags(flags(P, vp), R) <= R * R)
    s = np.zeros((classes, 3), dtype=np.int64)
    for c in range(classes):
        bt, bp = in_t & (T == c), in_p & (P == c)
        s[c] = [bt.sum(), bp.sum(), (bt & bp).sum()]
    tm = np.array([in_t.sum(), (in_t & ~vp & (P == T)).sum()], dtype=np.int64)
    return s, tm


# ------------------------------------------------------------------------------------------------------------- generators
CLASSES = 5
VOID = 255


def make_map(n, h, w, R, seed=0):
    """uint8 [n,h,w]: constant blocks of side 2R + 3 whose neighbours always differ in class (the centre of a whole block is
    further than R from every boundary: "far"; its column R is exactly R from the block's rim: R^2), every third block filled
    with per-pixel texture of the labels 0 .. CLASSES + 1 (two of them beyond the classes), and a void speck (255) in the corner
    region of every third block -- few enough that the clean blocks stay clean when void is an ordinary label."""
    rng = np.random.RandomState(1000 * seed + 131 * n + 17 * h + 3 * w + R)
    S = 2 * R + 3
    by, bx = np.arange(h) // S, np.arange(w) // S
    m = np.empty((n, h, w), dtype=np.uint8)
    for i in range(n):
        kind = (by[:, None] + bx[None, :] + i) % 3
        base = ((by[:, None] + 2 * bx[None, :] + i) % CLASSES).astype(np.uint8)
        tex = rng.randint(0, CLASSES + 2, size=(h, w)).astype(np.uint8)
        img = np.where(kind == 1, tex, base)
        speck = (kind == 2) & (np.arange(h)[:, None] % S == 1) & (np.arange(w)[None, :] % S == 1)
        img[speck] = VOID
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


def make_pred(truth, seed=0):
    """A prediction for a truth map: the truth moved one pixel right and two down, with a tenth of the pixels relabelled."""
    rng = np.random.RandomState(seed + 77)
    p = np.roll(np.roll(truth, 1, axis=2), 2, axis=1).copy()
    u = rng.rand(*p.shape)
    p[u < 0.1] = rng.randint(0, CLASSES + 1, size=int((u < 0.1).sum())).astype(p.dtype)
    return p


def kinds_present(d, R):
    """Which of the four kinds of value a d2 map holds: 0, strictly between, R^2 exactly, far."""
    return {"zero": bool((d == 0).any()), "between": bool(((d > 0) & (d < R * R)).any()), "cap": bool((d == R * R).any()),
            "far": bool((d == R * R + 1).any())}
