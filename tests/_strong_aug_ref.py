"""numpy restatement of the strong-augmentation pipeline of ``data.strong_views`` (the definition: INTEGRATION.md, "Phase 3").

Test infrastructure.  Every stage is written once, generically over the float type: ``run(images, params, np.float64)`` is the
reference the kernels are held to, ``run(..., np.float32)`` the same arithmetic in the kernels' precision -- the distance between
the two is what a float32 evaluation of this definition may legitimately differ by, and the GPU tests derive their bars from it.
All stages work on the 0..255 scale without rounding to uint8 in between; borders are reflect-101 everywhere.
"""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)

NOISE, BLUR, AFFINE, STAGE5, HSV = 1, 2, 4, 8, 16
(W_FLAGS, W_D4, W_BLUR_KIND, W_BLUR_K, W_MOTION_DIR, W_S5_KIND, W_KEY, W_SIGMA, W_AFFINE, W_S5_PARAMS, W_HSV) = \
    0, 1, 2, 3, 4, 5, 6, 8, 9, 15, 17


def reflect101(i, L):
    """Index into an axis of length L with reflect-101 borders (period 2(L-1), any distance; L == 1 reads index 0)."""
    i = np.asarray(i, dtype=np.int64)
    if L == 1:
        return np.zeros_like(i)
    p = 2 * (L - 1)
    i = np.mod(i, p)
    return np.where(i < L, i, p - i)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).  counter ``[...,4]``,
    key ``[...,2]`` unsigned 32-bit words -> ``[...,4]`` uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    m0, m1, w0, w1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), \
        np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & mask, p1 >> s32, p1 & mask
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + w0) & mask, (k[1] + w1) & mask]
    return np.stack(c, axis=-1).astype(np.uint32)


def d4_gather(img, code):
    """out[y, x] = img[source of (y, x)] under a D4 code of ``data.prepare_batch``'s convention (bit0 transpose, bit1 flip rows,
    bit2 flip columns, applied in that order)."""
    a = img
    if code & 1:
        a = a.transpose(1, 0, 2)
    if code & 2:
        a = a[::-1]
    if code & 4:
        a = a[:, ::-1]
    return np.ascontiguousarray(a)


def normals(h, w, key, dt):
    """z [h, w, 3]: Box-Muller on the four Philox words of counter (y*w + x, 0, 0, 0)."""
    ctr = np.zeros((h * w, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(h * w, dtype=np.uint32)
    r = philox4x32_10(ctr, np.broadcast_to(np.asarray(key, dtype=np.uint32), (h * w, 2)))
    u = ((r >> np.uint32(8)).astype(dt) + dt(0.5)) * dt(2.0 ** -24)
    two_pi = dt(6.283185307179586)
    a0 = np.sqrt(dt(-2.0) * np.log(u[:, 0]))
    a1 = np.sqrt(dt(-2.0) * np.log(u[:, 2]))
    z = np.stack([a0 * np.cos(two_pi * u[:, 1]), a0 * np.sin(two_pi * u[:, 1]), a1 * np.cos(two_pi * u[:, 3])], axis=-1)
    return z.reshape(h, w, 3).astype(dt)


def clamp(v, dt):
    return np.clip(v, dt(0.0), dt(255.0))


def add_noise(v, sigma, key, dt):
    h, w, _ = v.shape
    return clamp(v + dt(sigma) * normals(h, w, key, dt), dt)


def _shifted(v, dy, dx):
    h, w, _ = v.shape
    return v[reflect101(np.arange(h) + dy, h)][:, reflect101(np.arange(w) + dx, w)]


def blur(v, kind, k, direction, dt):
    r = k // 2
    if kind == 0:                                             # box
        acc = np.zeros_like(v)
        for i in range(-r, r + 1):
            for j in range(-r, r + 1):
                acc = acc + _shifted(v, i, j)
        return acc / dt(k * k)
    if kind == 1:                                             # per-channel median
        stack = np.stack([_shifted(v, i, j) for i in range(-r, r + 1) for j in range(-r, r + 1)], axis=0)
        return np.sort(stack, axis=0)[k * k // 2]
    dy = 0 if direction == 0 else 1                           # motion: horizontal, vertical, main diagonal, anti-diagonal
    dx = 0 if direction == 1 else (-1 if direction == 3 else 1)
    acc = np.zeros_like(v)
    for i in range(-r, r + 1):
        acc = acc + _shifted(v, i * dy, i * dx)
    return acc / dt(k)


def affine(v, m, dt):
    """Bilinear sample of v at M . (x, y, 1) for every output pixel; m: six numbers (row-major 2 x 3)."""
    h, w, _ = v.shape
    m = [dt(t) for t in m]
    y, x = np.meshgrid(np.arange(h).astype(dt), np.arange(w).astype(dt), indexing="ij")
    sx = m[0] * x + m[1] * y + m[2]
    sy = m[3] * x + m[4] * y + m[5]
    x0f, y0f = np.floor(sx), np.floor(sy)
    ax, ay = (sx - x0f)[..., None], (sy - y0f)[..., None]
    x0, x1 = reflect101(x0f.astype(np.int64), w), reflect101(x0f.astype(np.int64) + 1, w)
    y0, y1 = reflect101(y0f.astype(np.int64), h), reflect101(y0f.astype(np.int64) + 1, h)
    one = dt(1.0)
    out = (one - ay) * ((one - ax) * v[y0, x0] + ax * v[y0, x1]) + ay * ((one - ax) * v[y1, x0] + ax * v[y1, x1])
    return out.astype(dt)


def stage5_kernel(kind, p0, p1, dt):
    """The 3 x 3 kernel of sharpen (alpha, lightness) or emboss (alpha, strength), applied as a correlation."""
    a, p, one = dt(p0), dt(p1), dt(1.0)
    if kind == 0:
        k = np.full((3, 3), -a, dtype=dt)
        k[1, 1] = (one - a) + a * (dt(8.0) + p)
        return k
    return np.array([[a * (-one - p), a * -p, dt(0.0)], [a * -p, (one - a) + a, a * p], [dt(0.0), a * p, a * (one + p)]], dtype=dt)


def stage5(v, kind, p0, p1, dt):
    if kind == 2:                                             # brightness-contrast: v (1 + c) + 255 b
        return clamp(v * (dt(1.0) + dt(p1)) + dt(255.0) * dt(p0), dt)
    k = stage5_kernel(kind, p0, p1, dt)
    acc = np.zeros_like(v)
    for i in range(3):
        for j in range(3):
            acc = acc + k[i, j] * _shifted(v, i - 1, j - 1)
    return clamp(acc, dt)


def chroma(v):
    return v.max(axis=-1) - v.min(axis=-1)


def hsv_shift(v, dh, ds, dv, dt):
    """RGB -> HSV on OpenCV's 8-bit scales (h in [0,180), s and v in [0,255]; h = 0 where max == min), shift, back."""
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    mx, mn = v.max(axis=-1), v.min(axis=-1)
    delta = mx - mn
    safe = np.where(delta > 0, delta, dt(1.0))
    hh = np.where(mx == r, dt(30.0) * (g - b) / safe,
                  np.where(mx == g, dt(60.0) + dt(30.0) * (b - r) / safe, dt(120.0) + dt(30.0) * (r - g) / safe))
    hh = np.where(delta > 0, hh, dt(0.0)).astype(dt)
    ss = np.where(mx > 0, dt(255.0) * delta / np.where(mx > 0, mx, dt(1.0)), dt(0.0)).astype(dt)
    hh = hh + dt(dh)
    hh = hh - dt(180.0) * np.floor(hh / dt(180.0))
    ss = clamp(ss + dt(ds), dt)
    vv = clamp(mx + dt(dv), dt)
    h6 = hh / dt(30.0)
    fl = np.floor(h6)
    f = h6 - fl
    sector = fl.astype(np.int64) % 6
    s1 = ss / dt(255.0)
    one = dt(1.0)
    p, q, t = vv * (one - s1), vv * (one - s1 * f), vv * (one - s1 * (one - f))
    ro = np.choose(sector, [vv, q, p, p, t, vv])
    go = np.choose(sector, [t, vv, vv, q, p, p])
    bo = np.choose(sector, [p, p, t, vv, vv, q])
    return clamp(np.stack([ro, go, bo], axis=-1).astype(dt), dt)


def normalize(v, dt):
    """A.Normalize with ``data.prepare_batch``'s arithmetic: (v - mean255) * inv_std255, both constants rounded to fp32 first."""
    mean = (MEAN * np.float32(255.0)).astype(dt)
    inv = np.reciprocal(STD * np.float32(255.0), dtype=np.float32).astype(dt)
    return (v - mean) * inv


def run_sample(img_u8, ints, floats, dt):
    """One frame through the record ``(ints, floats)`` (the int32 / float32 readings of its 32 words).
    -> (normalised [h, w, 3] in ``dt``, chroma entering stage 6 [h, w] or None when that stage is off)."""
    flags = int(ints[W_FLAGS])
    v = d4_gather(img_u8, int(ints[W_D4])).astype(dt)
    if flags & NOISE:
        v = add_noise(v, floats[W_SIGMA], ints[W_KEY:W_KEY + 2].view(np.uint32), dt)
    if flags & BLUR:
        v = blur(v, int(ints[W_BLUR_KIND]), int(ints[W_BLUR_K]), int(ints[W_MOTION_DIR]), dt)
    if flags & AFFINE:
        v = affine(v, floats[W_AFFINE:W_AFFINE + 6], dt)
    if flags & STAGE5:
        v = stage5(v, int(ints[W_S5_KIND]), floats[W_S5_PARAMS], floats[W_S5_PARAMS + 1], dt)
    c = None
    if flags & HSV:
        c = chroma(v)
        v = hsv_shift(v, floats[W_HSV], floats[W_HSV + 1], floats[W_HSV + 2], dt)
    out = normalize(v, dt)
    assert out.dtype == dt, out.dtype
    return out, c


def run(images_u8, params, dt=np.float64):
    """images uint8 [n,h,w,3], params: ``data.StrongAugParams`` -> (normalised [n,h,w,3] in ``dt``, ill-conditioned mask [n,h,w]:
    pixels whose chroma entering the HSV stage is above 0 and below 0.5 level)."""
    outs, masks = [], []
    ints = np.ascontiguousarray(params.ints)
    for i in range(images_u8.shape[0]):
        o, c = run_sample(images_u8[i], ints[i], ints[i].view(np.float32), dt)
        outs.append(o)
        masks.append(np.zeros(o.shape[:2], dtype=bool) if c is None else (c > 0) & (c < 0.5))
    return np.stack(outs), np.stack(masks)
