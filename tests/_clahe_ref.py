"""numpy restatement of CLAHE in the two device augmentation pipelines (the definition: INTEGRATION.md, "CLAHE").

Test infrastructure, in the manner of ``_strong_aug_ref`` / ``_train_aug_ref`` (whose stages it reuses): the colour round trip
and the per-pixel blend are written once, generically over the float type -- ``np.float64`` is the reference the kernels are
held to, ``np.float32`` the same arithmetic in the kernels' precision -- and the per-tile table is integer arithmetic throughout.
``run_strong`` / ``run_train`` put the stage into the pipelines: stage 5 of a record of kind 3 is CLAHE, every other record goes
through the existing restatements' stages unchanged.
"""
import numpy as np

import _strong_aug_ref as S
import _train_aug_ref as T

CLAHE = 3                                                     # word 5
GRID, BINS = 8, 256
WHITE = (0.950456, 1.0, 1.088754)
RGB_TO_XYZ = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
# the nine numbers of the inverse as csrc/aug_common.h states them (float64 inverse, rounded once to fp32)
INVERSE_F32 = ("3.07993484", "-1.53715158", "-0.542783439", "-0.92123419", "1.87599003", "0.0452441797",
               "0.0528896824", "-0.204041332", "1.15115166")
FORWARD_F32 = ("0.433952749", "0.376219422", "0.18982783", "0.212670997", "0.715160012", "0.0721689984",
               "0.017757915", "0.109476522", "0.872765541")


def matrices(dt):
    """(forward, inverse) 3 x 3 in ``dt``: the D65 rows divided by the white point, and the float64 inverse of that, each
    rounded once to ``dt``."""
    m = np.array(RGB_TO_XYZ, dtype=np.float64) / np.array(WHITE, dtype=np.float64)[:, None]
    return m.astype(dt), np.linalg.inv(m).astype(dt)


def _f(t, dt):
    return np.where(t > dt(0.008856), np.cbrt(t), dt(7.787) * t + dt(16.0) / dt(116.0)).astype(dt)


def _f_inv(f, dt):
    t3 = f * f * f
    return np.where(t3 > dt(0.008856), t3, (f - dt(16.0) / dt(116.0)) / dt(7.787)).astype(dt)


def rgb_to_lab(v, dt):
    """v [..., 3] on the 0..255 scale in ``dt`` -> (L8, a, b), L8 = 2.55 L."""
    m, _ = matrices(dt)
    c = v / dt(255.0)
    big = np.power((np.maximum(c, dt(0.0)) + dt(0.055)) / dt(1.055), dt(2.4))
    lin = np.where(c <= dt(0.04045), c / dt(12.92), big).astype(dt)
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    fx = _f(m[0, 0] * r + m[0, 1] * g + m[0, 2] * b, dt)
    fy = _f(m[1, 0] * r + m[1, 1] * g + m[1, 2] * b, dt)
    fz = _f(m[2, 0] * r + m[2, 1] * g + m[2, 2] * b, dt)
    l8 = dt(2.55) * (dt(116.0) * fy - dt(16.0))
    return l8.astype(dt), (dt(500.0) * (fx - fy)).astype(dt), (dt(200.0) * (fy - fz)).astype(dt)


def lab_to_rgb(l8, a, b, dt):
    """The way back: [..., 3] on the 0..255 scale, clamped."""
    _, mi = matrices(dt)
    fy = (l8 / dt(2.55) + dt(16.0)) / dt(116.0)
    x, y, z = _f_inv(fy + a / dt(500.0), dt), _f_inv(fy, dt), _f_inv(fy - b / dt(200.0), dt)
    out = []
    for i in range(3):
        lin = (mi[i, 0] * x + mi[i, 1] * y + mi[i, 2] * z).astype(dt)
        big = dt(1.055) * np.power(np.maximum(lin, dt(0.0)), dt(1.0) / dt(2.4)) - dt(0.055)
        c = np.where(lin <= dt(0.0031308), dt(12.92) * lin, big).astype(dt)
        out.append(S.clamp(c * dt(255.0), dt))
    return np.stack(out, axis=-1).astype(dt)


def bins(l8):
    return np.clip(np.floor(l8 + l8.dtype.type(0.5)), 0, BINS - 1).astype(np.int64)


def tile_table(hist, clip, area):
    """One tile's table from its 256-bin histogram, in integers -> (lut uint8 [256], intermediates)."""
    hist = np.asarray(hist, dtype=np.int64).copy()
    assert hist.shape == (BINS,) and int(hist.sum()) == area
    limit = max(1, int(float(clip) * area / 256))
    excess = int(np.maximum(hist - limit, 0).sum())
    hist = np.minimum(hist, limit)
    share, rest = excess // BINS, excess % BINS
    hist += share
    step = 0
    if rest:
        step = max(BINS // rest, 1)
        i, left = 0, rest
        while i < BINS and left > 0:
            hist[i] += 1
            i += step
            left -= 1
    num = np.cumsum(hist) * 255
    q, rem = num // area, num % area
    q = q + ((2 * rem > area) | ((2 * rem == area) & (q % 2 == 1)))          # round half to even
    return np.minimum(q, 255).astype(np.uint8), dict(limit=limit, excess=excess, share=share, rest=rest, step=step)


def tables(k, clip):
    """k: the bins of one frame [h, w] -> (lut uint8 [8, 8, 256], per-tile intermediates [64])."""
    h, w = k.shape
    assert h % GRID == 0 and w % GRID == 0
    th, tw = h // GRID, w // GRID
    lut, info = np.zeros((GRID, GRID, BINS), dtype=np.uint8), []
    for ty in range(GRID):
        for tx in range(GRID):
            hist = np.bincount(k[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=BINS)
            lut[ty, tx], i = tile_table(hist, clip, th * tw)
            info.append(i)
    return lut, info


def _neighbours(coord, tile, dt):
    tf = coord.astype(dt) / dt(tile) - dt(0.5)
    fl = np.floor(tf)
    i = fl.astype(np.int64)
    return np.maximum(i, 0), np.minimum(i + 1, GRID - 1), (tf - fl).astype(dt)


def blend(k, lut, dt):
    """L8' [h, w]: the bilinear blend of the four neighbouring tiles' entries of the pixel's own bin."""
    h, w = k.shape
    y0, y1, ay = _neighbours(np.arange(h), h // GRID, dt)
    x0, x1, ax = _neighbours(np.arange(w), w // GRID, dt)
    y0, y1, ay = y0[:, None], y1[:, None], ay[:, None]
    x0, x1, ax = x0[None, :], x1[None, :], ax[None, :]
    t = lut.astype(dt)
    one = dt(1.0)
    out = (one - ay) * ((one - ax) * t[y0, x0, k] + ax * t[y0, x1, k]) + ay * ((one - ax) * t[y1, x0, k] + ax * t[y1, x1, k])
    return out.astype(dt)


def clahe(v, clip, dt, lut=None):
    """The stage on the stage-4 image v [h, w, 3] (0..255 scale, ``dt``) -> (image, lut used, L8, per-tile intermediates).
    ``lut``: a table to use in place of the frame's own."""
    l8, a, b = rgb_to_lab(v, dt)
    k = bins(l8)
    own, info = tables(k, clip)
    use = own if lut is None else lut
    out = lab_to_rgb(blend(k, use, dt), a, b, dt)
    assert out.dtype == dt and l8.dtype == dt
    return out, own, l8, info


def _finish(v, ints, floats, dt, lut):
    flags = int(ints[S.W_FLAGS])
    extra = dict(lut=None, l8=None, info=None)
    if flags & S.STAGE5:
        if int(ints[S.W_S5_KIND]) == CLAHE:
            v, own, l8, info = clahe(v, floats[S.W_S5_PARAMS], dt, lut)
            extra = dict(lut=own, l8=l8, info=info)
        else:
            v = S.stage5(v, int(ints[S.W_S5_KIND]), floats[S.W_S5_PARAMS], floats[S.W_S5_PARAMS + 1], dt)
    ill = np.zeros(v.shape[:2], dtype=bool)
    if flags & S.HSV:
        c = S.chroma(v)
        ill = (c > 0) & (c < 0.5)
        v = S.hsv_shift(v, floats[S.W_HSV], floats[S.W_HSV + 1], floats[S.W_HSV + 2], dt)
    out = S.normalize(v, dt)
    assert out.dtype == dt
    return out, ill, extra


def _stage4_strong(img_u8, ints, floats, dt):
    flags = int(ints[S.W_FLAGS])
    v = S.d4_gather(img_u8, int(ints[S.W_D4])).astype(dt)
    if flags & S.NOISE:
        v = S.add_noise(v, floats[S.W_SIGMA], ints[S.W_KEY:S.W_KEY + 2].view(np.uint32), dt)
    if flags & S.BLUR:
        v = S.blur(v, int(ints[S.W_BLUR_KIND]), int(ints[S.W_BLUR_K]), int(ints[S.W_MOTION_DIR]), dt)
    if flags & S.AFFINE:
        v = S.affine(v, floats[S.W_AFFINE:S.W_AFFINE + 6], dt)
    return v


def _stage4_train(img_u8, mask_u8, ints, floats, sigma, dt):
    flags = int(ints[S.W_FLAGS])
    code = int(ints[S.W_D4])
    h, w = img_u8.shape[:2]
    v = S.d4_gather(img_u8, code).astype(dt)
    if flags & S.NOISE:
        v = S.add_noise(v, floats[S.W_SIGMA], ints[S.W_KEY:S.W_KEY + 2].view(np.uint32), dt)
    if flags & S.BLUR:
        v = S.blur(v, int(ints[S.W_BLUR_KIND]), int(ints[S.W_BLUR_K]), int(ints[S.W_MOTION_DIR]), dt)
    pos = T.positions(ints, floats, h, w, sigma, dt)
    m = None if mask_u8 is None else S.d4_gather(mask_u8[..., None], code)[..., 0]
    if pos is not None:
        v = T.sample_bilinear(v, pos[0], pos[1], dt)
        if m is not None:
            my, mx = T.nearest(pos[0], pos[1], h, w)
            m = m[my, mx]
    return v, (None if m is None else m.astype(np.int64))


def _collect(rows, n, h, w):
    outs, ills, luts, l8s, infos = [], [], [], [], []
    for out, ill, extra in rows:
        outs.append(out)
        ills.append(ill)
        luts.append(extra["lut"] if extra["lut"] is not None else np.zeros((GRID, GRID, BINS), dtype=np.uint8))
        l8s.append(extra["l8"] if extra["l8"] is not None else np.full((h, w), np.nan, dtype=out.dtype))
        infos.append(extra["info"])
    return dict(img=np.stack(outs), ill=np.stack(ills), lut=np.stack(luts), l8=np.stack(l8s), info=infos)


def run_strong(images_u8, params, dt=np.float64, luts=None):
    """images uint8 [n,h,w,3], params: ``data.StrongAugParams`` -> dict(img [n,h,w,3] normalised in ``dt``, ill [n,h,w] (hue
    decided by rounding noise), lut [n,8,8,256] (the frames' own tables; zeros off CLAHE), l8 [n,h,w] (the stage-4 lightness; NaN
    off CLAHE), info).  ``luts`` [n,8,8,256]: tables to blend from in place of the frames' own."""
    n, h, w, _ = images_u8.shape
    ints = np.ascontiguousarray(params.ints)
    rows = []
    for i in range(n):
        fl = ints[i].view(np.float32)
        rows.append(_finish(_stage4_strong(images_u8[i], ints[i], fl, dt), ints[i], fl, dt, None if luts is None else luts[i]))
    return _collect(rows, n, h, w)


def run_train(images_u8, masks_u8, params, dt=np.float64, luts=None, sigma=6.0):
    """As ``run_strong`` for ``data.TrainAugParams``; the dict also holds mask [n,h,w] int64 (or None)."""
    n, h, w, _ = images_u8.shape
    ints = np.ascontiguousarray(params.ints)
    rows, ms = [], []
    for i in range(n):
        fl = ints[i].view(np.float32)
        v, m = _stage4_train(images_u8[i], None if masks_u8 is None else masks_u8[i], ints[i], fl, sigma, dt)
        rows.append(_finish(v, ints[i], fl, dt, None if luts is None else luts[i]))
        ms.append(m)
    out = _collect(rows, n, h, w)
    out["mask"] = None if masks_u8 is None else np.stack(ms)
    return out


def boundary_distance(l8):
    """Distance of L8 from the nearest bin boundary (k + 0.5); beyond the clamped ends there is none."""
    t = l8.astype(np.float64) + 0.5
    d = np.abs(t - np.round(t))
    return np.where((l8 < -0.5) | (l8 > 255.5), np.inf, d)
