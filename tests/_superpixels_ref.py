"""The numpy mirror of the superpixel rule of include/udaseg.h (csrc/superpixels.hip), vectorised, with the frames the tests share.

Everything is integer arithmetic in int64, so the mirror and the device agree bit for bit or one of them is wrong.  Nothing here
needs a GPU.  The brute-force restatements (a per-pixel loop over the 9 candidates, a flood fill and a sequential raster-order
absorb) live here too; tests/test_superpixels_host.py holds the mirror to them on tiny shapes."""
import functools

import numpy as np

I64_MAX = np.iinfo(np.int64).max


def grid_of(h, w, S):
    return -(-h // S), -(-w // S)


# ------------------------------------------------------------------------------------------------------------------- SLIC
def start_centres(frame, S):
    """int64 [K,6] of one frame [h,w,3]."""
    h, w, _ = frame.shape
    gh, gw = grid_of(h, w, S)
    gy, gx = np.divmod(np.arange(gh * gw), gw)
    y0 = np.minimum(gy * S + S // 2, h - 1)
    x0 = np.minimum(gx * S + S // 2, w - 1)
    c = np.zeros((gh * gw, 6), dtype=np.int64)
    c[:, 0], c[:, 1] = 16 * y0, 16 * x0
    c[:, 2:5] = 16 * frame[y0, x0, :].astype(np.int64)
    return c


def assign(frame, centres, S, m):
    """int64 [h,w]: the cluster of every pixel (the smallest D over the up to 9 cells around its own, ties to the smallest k)."""
    h, w, _ = frame.shape
    gh, gw = grid_of(h, w, S)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    gy, gx = y // S, x // S
    col = 16 * frame.astype(np.int64)
    D = np.full((9, h, w), I64_MAX, dtype=np.int64)
    ks = np.zeros((9, h, w), dtype=np.int64)
    j = 0
    for dy in (-1, 0, 1):                                     # ascending k: argmin takes the first minimum
        for dx in (-1, 0, 1):
            cy, cx = gy + dy, gx + dx
            ok = (cy >= 0) & (cy < gh) & (cx >= 0) & (cx < gw)
            k = np.where(ok, cy * gw + cx, 0)
            c = centres[k]
            dc = ((col - c[..., 2:5]) ** 2).sum(-1)
            ds = (16 * y - c[..., 0]) ** 2 + (16 * x - c[..., 1]) ** 2
            D[j] = np.where(ok, S * S * dc + m * m * ds, I64_MAX)
            ks[j] = k
            j += 1
    best = D.argmin(0)
    return np.take_along_axis(ks, best[None], 0)[0]


def update(frame, labels, centres):
    """The centres after one update: (16 sum + count // 2) // count, a cluster without a pixel keeps its centre; count stored."""
    h, w, _ = frame.shape
    K = centres.shape[0]
    lab = labels.reshape(-1)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    comps = [y.reshape(-1), x.reshape(-1)] + [frame[..., i].reshape(-1).astype(np.int64) for i in range(3)]
    cnt = np.bincount(lab, minlength=K).astype(np.int64)
    out = centres.copy()
    has = cnt > 0
    for i, v in enumerate(comps):
        s = np.zeros(K, dtype=np.int64)
        np.add.at(s, lab, v)
        assert s.max(initial=0) < 2 ** 31                     # the device keeps the sums in int32
        out[has, i] = (16 * s[has] + cnt[has] // 2) // cnt[has]
    out[:, 5] = cnt
    return out


def components(lab):
    """int64 [h,w]: the first raster index of every pixel's 4-connected component of equal values (a union-find over the equal
    neighbour pairs, the larger root always linked to the smaller)."""
    h, w = lab.shape
    idx = np.arange(h * w).reshape(h, w)
    eh, ev = lab[:, :-1] == lab[:, 1:], lab[:-1, :] == lab[1:, :]
    a = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]]).tolist()
    b = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]]).tolist()
    par = list(range(h * w))
    for p, q in zip(a, b):
        while par[p] != p:
            par[p] = par[par[p]]
            p = par[p]
        while par[q] != q:
            par[q] = par[par[q]]
            q = par[q]
        if p < q:
            par[q] = p
        elif q < p:
            par[p] = q
    par = np.asarray(par, dtype=np.int64)
    while True:
        nxt = par[par]
        if np.array_equal(nxt, par):
            break
        par = nxt
    return par.reshape(h, w)


def connect(lab, min_area=0):
    """(ids int64 [h,w], counts [4], longest chain) of one image's cluster map."""
    h, w = lab.shape
    root = components(lab).reshape(-1)
    flat = lab.reshape(-1)
    roots = np.flatnonzero(root == np.arange(h * w))
    area = np.bincount(root, minlength=h * w)
    main = {}
    for r in roots.tolist():                                  # ascending roots: a later one must be strictly larger to win
        k = int(flat[r])
        best = main.get(k)
        if best is None or (best != 0 and area[r] > area[best]):
            main[k] = r
    fin = np.full(h * w, -1, dtype=np.int64)
    depth = np.zeros(h * w, dtype=np.int64)
    absorbed = 0
    for r in roots.tolist():
        k = int(flat[r])
        if main[k] == r and (area[r] >= min_area or r == 0):
            fin[r] = k
        else:
            q = r - 1 if r % w > 0 else r - w
            fin[r] = fin[root[q]]
            depth[r] = depth[root[q]] + 1
            absorbed += 1
    ids = fin[root].reshape(h, w)
    counts = np.array([len(roots), absorbed, int((ids != lab).sum()), len(np.unique(ids))], dtype=np.int64)
    return ids, counts, int(depth.max())


def slic(frames, S=16, m=10, T=10, min_area=0, info=None):
    """(ids int32 [n,h,w], centres int32 [n,K,6], counts int64 [n,4]) of uint8 frames [n,h,w,3].  ``info``: a dict that receives
    the labels before the connect step and the longest absorb chain per image."""
    n, h, w, _ = frames.shape
    gh, gw = grid_of(h, w, S)
    ids = np.zeros((n, h, w), dtype=np.int32)
    cen = np.zeros((n, gh * gw, 6), dtype=np.int32)
    counts = np.zeros((n, 4), dtype=np.int64)
    labels, chains = [], []
    for i in range(n):
        c = start_centres(frames[i], S)
        for _ in range(T):
            lab = assign(frames[i], c, S, m)
            c = update(frames[i], lab, c)
        assert c[:, 5].max() <= 9 * S * S
        out, counts[i], chain = connect(lab, min_area)
        ids[i], cen[i] = out, c
        labels.append(lab)
        chains.append(chain)
    if info is not None:
        info["labels"], info["chains"] = np.stack(labels), chains
    return ids, cen, counts


# -------------------------------------------------------------------------------------------------------- brute-force forms
def assign_brute(frame, centres, S, m):
    h, w, _ = frame.shape
    gh, gw = grid_of(h, w, S)
    out = np.zeros((h, w), dtype=np.int64)
    for y in range(h):
        for x in range(w):
            best, bk = None, None
            for cy in range(y // S - 1, y // S + 2):
                for cx in range(x // S - 1, x // S + 2):
                    if not (0 <= cy < gh and 0 <= cx < gw):
                        continue
                    k = cy * gw + cx
                    Y, X, C0, C1, C2 = (int(v) for v in centres[k, :5])
                    c = [int(v) for v in frame[y, x]]
                    D = S * S * ((16 * c[0] - C0) ** 2 + (16 * c[1] - C1) ** 2 + (16 * c[2] - C2) ** 2) \
                        + m * m * ((16 * y - Y) ** 2 + (16 * x - X) ** 2)
                    if best is None or D < best:
                        best, bk = D, k
            out[y, x] = bk
    return out


def connect_brute(lab, min_area=0):
    """Flood fill in raster order, then the absorb rule applied to the components in the order of their first pixels."""
    h, w = lab.shape
    comp = -np.ones((h, w), dtype=np.int64)
    info = []                                                 # per component in raster order of its first pixel: (label, area)
    for y in range(h):
        for x in range(w):
            if comp[y, x] >= 0:
                continue
            c, k, stack, area = len(info), lab[y, x], [(y, x)], 0
            comp[y, x] = c
            while stack:
                py, px = stack.pop()
                area += 1
                for qy, qx in ((py - 1, px), (py + 1, px), (py, px - 1), (py, px + 1)):
                    if 0 <= qy < h and 0 <= qx < w and comp[qy, qx] < 0 and lab[qy, qx] == k:
                        comp[qy, qx] = c
                        stack.append((qy, qx))
            info.append((int(k), area, y, x))
    final = []
    for c, (k, area, y, x) in enumerate(info):
        same = [(a, -d) for d, (kk, a, _, _) in enumerate(info) if kk == k]
        if info[0][0] == k:
            is_main = c == 0
        else:
            is_main = (area, -c) == max(same)
        if is_main and (area >= min_area or c == 0):
            final.append(k)
        else:
            final.append(final[comp[y, x - 1] if x > 0 else comp[y - 1, 0]])
    return np.asarray(final, dtype=np.int64)[comp]


# -------------------------------------------------------------------------------------------------------- vote, mean, select
def vote(ids, masks, C, ignore_index=255, min_share=0.0, min_cover=0.0, void=None, K=None):
    """(uint8 [n,h,w], counts int64 [n,3])."""
    ids = np.asarray(ids).astype(np.int64)
    m = np.asarray(masks).astype(np.int64)
    m = np.where((m < 0) | (m > 255), 255, m)
    void = (255 if ignore_index is None else ignore_index) if void is None else void
    K = int(ids.max()) + 1 if K is None else K
    share, cover = float(np.float32(min_share)), float(np.float32(min_cover))
    out = np.zeros(ids.shape, dtype=np.uint8)
    counts = np.zeros((ids.shape[0], 3), dtype=np.int64)
    for i in range(ids.shape[0]):
        lab = (m[i] < C) if ignore_index is None else ((m[i] < C) & (m[i] != ignore_index))
        T = np.bincount(ids[i][lab] * C + m[i][lab], minlength=K * C).reshape(K, C)
        size = np.bincount(ids[i].reshape(-1), minlength=K)
        labelled = T.sum(1)
        win = T.argmax(1)                                     # the first maximum: ties to the smallest class
        top = T.max(1)
        ok = (labelled > 0) & (top.astype(np.float64) >= share * labelled.astype(np.float64)) \
            & (labelled.astype(np.float64) >= cover * size.astype(np.float64))
        dec = np.where(ok, win, -1)[ids[i]]
        out[i] = np.where(dec >= 0, dec, void).astype(np.uint8)
        counts[i] = [int((lab & (dec >= 0) & (dec != m[i])).sum()), int((~lab & (dec >= 0)).sum()), int((lab & (dec < 0)).sum())]
    return out, counts


def mean(values, ids, K):
    """fp32 [n,K]."""
    v = np.asarray(values, dtype=np.float32)
    out = np.full((v.shape[0], K), -1.0, dtype=np.float32)
    for i in range(v.shape[0]):
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(v[i]) & (v[i] >= 0) & (v[i] <= 1)
        q = np.rint(v[i][ok] * np.float32(16777216.0)).astype(np.int64)
        s = np.zeros(K, dtype=np.int64)
        np.add.at(s, ids[i][ok], q)
        c = np.bincount(ids[i][ok], minlength=K).astype(np.int64)
        has = c > 0
        out[i, has] = (s[has].astype(np.float64) / (c[has].astype(np.float64) * 16777216.0)).astype(np.float32)
    return out


def select(key, ids, K, items, into=None):
    """(mask uint8 [n,h,w], counts int64 [n,2]): the ``items`` superpixels with the smallest mean key, every tie kept."""
    table = mean(key, ids, K)
    mask = np.zeros(ids.shape, dtype=np.uint8) if into is None else into.copy()
    counts = np.zeros((ids.shape[0], 2), dtype=np.int64)
    for i in range(ids.shape[0]):
        cand = table[i] >= 0
        vals = np.sort(table[i][cand])
        thr = -np.inf if items == 0 else (vals[items - 1] if items <= len(vals) else np.inf)
        picked = cand & (table[i] <= thr)
        counts[i] = [int(picked.sum()), int(cand.sum())]
        mask[i] |= picked[ids[i]].astype(np.uint8)
    return mask, counts


def outline(ids):
    e = np.zeros(ids.shape, dtype=bool)
    e[:, :, :-1] |= ids[:, :, :-1] != ids[:, :, 1:]
    e[:, :-1, :] |= ids[:, :-1, :] != ids[:, 1:, :]
    return e.astype(np.uint8)


def n_components(ids):
    """The 4-connected components of equal ids of one image."""
    r = components(np.asarray(ids, dtype=np.int64))
    return int((r.reshape(-1) == np.arange(r.size)).sum())


# ------------------------------------------------------------------------------------------------------------- the frames
# well separated colours: two regions differ by at least 48 in some channel
PALETTE = np.array([[r, g, b] for r in (16, 80, 144, 208) for g in (24, 120, 216) for b in (40, 200)], dtype=np.uint8)


def voronoi(n, h, w, seeds, noise=0, seed=0):
    """(frames uint8 [n,h,w,3], regions uint8 [n,h,w]): piecewise-constant Voronoi frames of ``seeds`` sites with distinct palette
    colours, plus uniform integer noise in [-noise, noise]; every image of a batch has its own sites."""
    frames = np.zeros((n, h, w, 3), dtype=np.uint8)
    regions = np.zeros((n, h, w), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    for i in range(n):
        rng = np.random.default_rng(1000 * seed + 17 * i + h + w)
        sy, sx = rng.uniform(0, h, seeds), rng.uniform(0, w, seeds)
        d = (y[None] - sy[:, None, None]) ** 2 + (x[None] - sx[:, None, None]) ** 2
        reg = d.argmin(0)
        colour = PALETTE[rng.permutation(len(PALETTE))[:seeds]]
        f = colour[reg].astype(np.int64)
        if noise:
            f = np.clip(f + rng.integers(-noise, noise + 1, f.shape), 0, 255)
        frames[i], regions[i] = f.astype(np.uint8), reg.astype(np.uint8)
    return frames, regions


def constant(n, h, w):
    return np.stack([np.full((h, w, 3), 90 + 40 * i, dtype=np.uint8) for i in range(n)])


def random_frame(n, h, w, seed=0):
    return np.random.default_rng(500 + seed + h * w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


# name -> (n, h, w, S, kind, arguments of the generator); m = 10 and T = 10 everywhere
CASES = {
    "one_cluster": (1, 9, 9, 16, "voronoi", dict(seeds=2)),
    "one_grid_row": (1, 5, 40, 8, "voronoi", dict(seeds=3)),
    "ragged_pair": (2, 37, 53, 8, "voronoi", dict(seeds=5, noise=3)),
    "clean_64": (1, 64, 64, 16, "voronoi", dict(seeds=3)),
    "many_clusters": (1, 70, 130, 4, "voronoi", dict(seeds=9, noise=2)),
    "fragments": (1, 150, 200, 8, "voronoi", dict(seeds=12, noise=8)),
    "random": (1, 48, 64, 8, "random", dict()),
    "constant": (1, 40, 50, 8, "constant", dict()),
    "max_step": (1, 130, 70, 64, "voronoi", dict(seeds=6, noise=2)),
}
ROUND_TRIP = {                                               # noise-free, regions larger than a cell: the vote returns the regions
    "clean_64": (1, 64, 64, 16, 3), "clean_64_s8": (2, 64, 64, 8, 6), "one_grid_row": (1, 5, 40, 8, 3),
}
FRAGMENT_HEAVY = ("fragments", "random")
COMPACTNESS, ITERATIONS = 10, 10


@functools.lru_cache(maxsize=None)
def case(name):
    """(frames, regions or None, S) of a named case; made once, read-only."""
    n, h, w, S, kind, kw = CASES[name]
    if kind == "voronoi":
        frames, regions = voronoi(n, h, w, **kw)
    elif kind == "constant":
        frames, regions = constant(n, h, w), None
    else:
        frames, regions = random_frame(n, h, w), None
    frames.setflags(write=False)
    return frames, regions, S


@functools.lru_cache(maxsize=None)
def reference(name, min_area=0):
    """The mirror's (ids, centres, counts, info) of a named case at the shared compactness and iterations; made once."""
    frames, _, S = case(name)
    info = {}
    ids, cen, counts = slic(frames, S, COMPACTNESS, ITERATIONS, min_area, info)
    for a in (ids, cen, counts):
        a.setflags(write=False)
    return ids, cen, counts, info


def masks_for(name, classes=5):
    """uint8 masks of a case: blocks of classes with void (255) speckles and a value >= classes, different per image."""
    n, h, w = CASES[name][:3]
    rng = np.random.default_rng(h * 7 + w)
    y, x = np.mgrid[0:h, 0:w]
    m = np.stack([((y // 6 + x // 9 + i) % classes) for i in range(n)]).astype(np.uint8)
    m[rng.random(m.shape) < 0.25] = 255
    m[rng.random(m.shape) < 0.05] = classes + 1
    return m


def values_for(name):
    """fp32 values of a case: uniform in [0, 1] with -1, NaN, inf, 1.5 and exact 0 / 1 planted."""
    n, h, w = CASES[name][:3]
    rng = np.random.default_rng(h * 11 + w)
    v = rng.random((n, h, w)).astype(np.float32)
    r = rng.random(v.shape)
    v[r < 0.2] = -1.0
    v[(r >= 0.2) & (r < 0.22)] = np.nan
    v[(r >= 0.22) & (r < 0.24)] = np.inf
    v[(r >= 0.24) & (r < 0.26)] = 1.5
    v[(r >= 0.26) & (r < 0.28)] = 0.0
    v[(r >= 0.28) & (r < 0.30)] = 1.0
    return v
