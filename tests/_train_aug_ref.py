"""numpy restatement of the labelled training augmentation of ``data.train_batch`` (the definition: INTEGRATION.md, "Training
augmentation").

Test infrastructure, in the manner of ``_strong_aug_ref`` (whose stages it shares): every stage is written once, generically
over the float type; ``run(..., np.float64)`` is the reference the kernels are held to, ``run(..., np.float32)`` the same
arithmetic in the kernels' precision.  Besides the image it returns the mask, the source positions ``r`` of the composed gather
and the pixels whose hue is decided by rounding noise; ``tie_band`` marks the pixels whose nearest label is decided by rounding
noise (``r + 0.5`` within ``band`` of an integer), ``mask_candidates`` the labels on either side of such a tie.
"""
import math

import numpy as np

import _strong_aug_ref as S

DISTORT = 32
OPTICAL, GRID, ELASTIC = 1, 2, 3
W_KIND, W_OPTICAL, W_GRID_X, W_GRID_Y, W_ALPHA, W_EKEY = 32, 33, 36, 42, 48, 50


def gaussian_weights(sigma):
    """radius R = ceil(3 sigma); exp(-i^2 / (2 sigma^2)) normalised to sum 1 over the 2R + 1 taps in float64, rounded once to
    fp32 (the values the kernel receives)."""
    radius = int(math.ceil(3.0 * sigma))
    i = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-i * i / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(np.float32), radius


def raw_field(h, w, key, dt):
    """[h, w, 2]: (2 u0 - 1, 2 u1 - 1) from the first two words of Philox4x32-10 at counter (y w + x, 1, 0, 0)."""
    ctr = np.zeros((h * w, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(h * w, dtype=np.uint32)
    ctr[:, 1] = 1
    r = S.philox4x32_10(ctr, np.broadcast_to(np.asarray(key, dtype=np.uint32), (h * w, 2)))
    u = ((r[:, :2] >> np.uint32(8)).astype(dt) + dt(0.5)) * dt(2.0 ** -24)
    return (dt(2.0) * u - dt(1.0)).reshape(h, w, 2).astype(dt)


def smooth(raw, weights, radius, dt):
    """Separable Gaussian with reflect-101 at any distance: the horizontal pass, then the vertical one, taps in ascending order."""
    h, w, _ = raw.shape
    wt = weights.astype(dt)
    acc = np.zeros_like(raw)
    for k in range(2 * radius + 1):
        acc = acc + wt[k] * raw[:, S.reflect101(np.arange(w) + (k - radius), w)]
    out = np.zeros_like(raw)
    for k in range(2 * radius + 1):
        out = out + wt[k] * acc[S.reflect101(np.arange(h) + (k - radius), h)]
    return out.astype(dt)


def elastic_field(ints, h, w, sigma, dt):
    weights, radius = gaussian_weights(sigma)
    return smooth(raw_field(h, w, ints[W_EKEY:W_EKEY + 2].view(np.uint32), dt), weights, radius, dt)


def _grid_axis(coord, side, steps, dt):
    cell = side // 5
    i = np.minimum(coord // cell, 5)                          # the last cell takes what remains of the axis
    start = [dt(0.0)]
    for k in range(5):
        start.append(start[k] + dt(cell) * dt(steps[k]))
    start, steps = np.array(start, dtype=dt), np.array([dt(s) for s in steps], dtype=dt)
    return start[i] + (coord - i * cell).astype(dt) * steps[i]


def positions(ints, floats, h, w, sigma, dt):
    """Source position r = M (q(p), 1) of every output pixel -> (rx, ry) [h, w] in ``dt``, or None without stage 4 / 4b."""
    flags = int(ints[S.W_FLAGS])
    kind = int(ints[W_KIND]) if flags & DISTORT else 0
    if not (flags & S.AFFINE or kind):
        return None
    yi, xi = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    fx, fy = xi.astype(dt), yi.astype(dt)
    qx, qy = fx, fy
    if kind == OPTICAL:
        k, dx, dy = (dt(v) for v in floats[W_OPTICAL:W_OPTICAL + 3])
        cx, cy = dt(w - 1) * dt(0.5) + dx, dt(h - 1) * dt(0.5) + dy
        ex, ey = fx - cx, fy - cy
        u, v = ex / dt(w), ey / dt(h)
        r2 = u * u + v * v
        f = dt(1.0) + k * r2 + k * r2 * r2
        qx, qy = cx + ex * f, cy + ey * f
    elif kind == GRID:
        qx = _grid_axis(xi, w, floats[W_GRID_X:W_GRID_X + 6], dt)
        qy = _grid_axis(yi, h, floats[W_GRID_Y:W_GRID_Y + 6], dt)
    elif kind == ELASTIC:
        g = elastic_field(ints, h, w, sigma, dt)
        alpha = dt(floats[W_ALPHA])
        qx, qy = fx + alpha * g[..., 0], fy + alpha * g[..., 1]
    if flags & S.AFFINE:
        m = [dt(t) for t in floats[S.W_AFFINE:S.W_AFFINE + 6]]
        rx = m[0] * qx + m[1] * qy + m[2]
        ry = m[3] * qx + m[4] * qy + m[5]
    else:
        rx, ry = qx, qy
    return rx.astype(dt), ry.astype(dt)


def sample_bilinear(v, rx, ry, dt):
    h, w, _ = v.shape
    x0f, y0f = np.floor(rx), np.floor(ry)
    ax, ay = (rx - x0f)[..., None], (ry - y0f)[..., None]
    x0, x1 = S.reflect101(x0f.astype(np.int64), w), S.reflect101(x0f.astype(np.int64) + 1, w)
    y0, y1 = S.reflect101(y0f.astype(np.int64), h), S.reflect101(y0f.astype(np.int64) + 1, h)
    one = dt(1.0)
    out = (one - ay) * ((one - ax) * v[y0, x0] + ax * v[y0, x1]) + ay * ((one - ax) * v[y1, x0] + ax * v[y1, x1])
    return out.astype(dt)


def nearest(rx, ry, h, w):
    """Nearest source pixel: (floor(r_x + 0.5), floor(r_y + 0.5)), reflect-101."""
    half = rx.dtype.type(0.5)
    return S.reflect101(np.floor(ry + half).astype(np.int64), h), S.reflect101(np.floor(rx + half).astype(np.int64), w)


def run_sample(img_u8, mask_u8, ints, floats, sigma, dt):
    """One frame (and its mask, or None) through the 64-word record -> (normalised [h,w,3] in ``dt``, mask [h,w] int64 or None,
    r [h,w,2] in ``dt`` (x, y), chroma entering stage 6 or None)."""
    flags = int(ints[S.W_FLAGS])
    code = int(ints[S.W_D4])
    h, w = img_u8.shape[:2]
    v = S.d4_gather(img_u8, code).astype(dt)
    if flags & S.NOISE:
        v = S.add_noise(v, floats[S.W_SIGMA], ints[S.W_KEY:S.W_KEY + 2].view(np.uint32), dt)
    if flags & S.BLUR:
        v = S.blur(v, int(ints[S.W_BLUR_KIND]), int(ints[S.W_BLUR_K]), int(ints[S.W_MOTION_DIR]), dt)
    pos = positions(ints, floats, h, w, sigma, dt)
    m = None if mask_u8 is None else S.d4_gather(mask_u8[..., None], code)[..., 0]
    if pos is None:
        yi, xi = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        r = np.stack([xi.astype(dt), yi.astype(dt)], axis=-1)
    else:
        v = sample_bilinear(v, pos[0], pos[1], dt)
        r = np.stack(pos, axis=-1)
        if m is not None:
            my, mx = nearest(pos[0], pos[1], h, w)
            m = m[my, mx]
    if flags & S.STAGE5:
        v = S.stage5(v, int(ints[S.W_S5_KIND]), floats[S.W_S5_PARAMS], floats[S.W_S5_PARAMS + 1], dt)
    c = None
    if flags & S.HSV:
        c = S.chroma(v)
        v = S.hsv_shift(v, floats[S.W_HSV], floats[S.W_HSV + 1], floats[S.W_HSV + 2], dt)
    out = S.normalize(v, dt)
    assert out.dtype == dt and r.dtype == dt, (out.dtype, r.dtype)
    return out, (None if m is None else m.astype(np.int64)), r, c


def run(images_u8, masks_u8, params, dt=np.float64, sigma=6.0):
    """images uint8 [n,h,w,3], masks uint8 [n,h,w] or None, params: ``data.TrainAugParams`` -> (normalised [n,h,w,3] in ``dt``,
    masks [n,h,w] int64 or None, r [n,h,w,2] in ``dt``, hue-ill mask [n,h,w]: chroma entering the HSV stage above 0 and below
    0.5 level)."""
    outs, ms, rs, ill = [], [], [], []
    ints = np.ascontiguousarray(params.ints)
    for i in range(images_u8.shape[0]):
        o, m, r, c = run_sample(images_u8[i], None if masks_u8 is None else masks_u8[i], ints[i], ints[i].view(np.float32), sigma, dt)
        outs.append(o)
        ms.append(m)
        rs.append(r)
        ill.append(np.zeros(o.shape[:2], dtype=bool) if c is None else (c > 0) & (c < 0.5))
    return np.stack(outs), (None if masks_u8 is None else np.stack(ms)), np.stack(rs), np.stack(ill)


def band_width(r64, r32, h, w):
    """Per sample: max(4 x max |r_f32 - r_f64|, 2 ulp of fp32 at max(H, W))."""
    dev = np.abs(r32.astype(np.float64) - r64).reshape(r64.shape[0], -1).max(axis=1)
    return np.maximum(4.0 * dev, 2.0 * float(np.spacing(np.float32(max(h, w)))))


def tie_band(r64, band):
    """[n,h,w] bool: r_x + 0.5 or r_y + 0.5 within ``band[n]`` of an integer."""
    t = r64 + 0.5
    d = np.abs(t - np.round(t))
    return (d <= band[:, None, None, None]).any(axis=-1)


def mask_candidates(mask_u8, code, r64, band):
    """The labels on either side of a tie for one sample: [4,h,w] int64, the D4-gathered mask at
    (floor(r + 0.5 -/+ band)) per axis."""
    h, w = mask_u8.shape
    m = S.d4_gather(mask_u8[..., None], code)[..., 0]
    out = []
    for sy in (-band, band):
        for sx in (-band, band):
            my = S.reflect101(np.floor(r64[..., 1] + 0.5 + sy).astype(np.int64), h)
            mx = S.reflect101(np.floor(r64[..., 0] + 0.5 + sx).astype(np.int64), w)
            out.append(m[my, mx].astype(np.int64))
    return np.stack(out)
